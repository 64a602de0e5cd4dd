"""Training targets without a GPU: the numpy restatement of tests/targets_ref.py against the known answers of
Philox4x32-10 and against rows worked by hand, every argument check of mask_tokens / lm_labels / batch_encode_mlm that
comes before a device call, and what the two C calls refuse before they look for a device.  The kernels are compared
with the restatement in tests/test_gpu_targets.py."""
import numpy as np
import pytest

import targets_ref as T

import hutoken_amd
from hutoken_amd import _capi

I = -100  # the ignore index of the worked rows
M = 99    # their mask id
ONE = 2**32
ALWAYS = dict(seed=7, select_below=ONE, mask_below=ONE, random_below=ONE, mask_id=M)  # every eligible column becomes M


# ---- the generator ----------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """The vectors of the Random123 distribution (kat_vectors: philox4x32 10)."""
    cases = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for counter, key, want in cases:
        assert tuple(int(x) for x in T.philox4x32_10(counter, key)) == want
    # all three at once: the restatement is the same function element by element
    got = T.philox4x32_10([np.array(x) for x in zip(*(c for c, _k, _w in cases))], [np.array(x) for x in zip(*(k for _c, k, _w in cases))])
    assert [tuple(int(x[i]) for x in got) for i in range(3)] == [w for _c, _k, w in cases]


def test_draws_of_seed_1234():
    rows, cols = np.meshgrid(np.arange(400), np.arange(512), indexing="ij")
    u0, u1, u2, _u3 = T.draw(1234, rows, cols, T.COLUMN)
    selected = u0 < T.threshold(0.15)
    assert int(selected.sum()) == 30643  # of 204800: 0.1496, -0.48 sigma from 0.15
    masked = u1 < T.threshold(0.8)
    assert round(float(masked.mean()), 4) == 0.8008  # of all columns; of the selected ones 24555, 0.8013
    assert int(masked[selected].sum()) == 24555
    ids = (u2 * np.uint64(50257)) >> np.uint64(32)
    assert int(ids.min()) == 0 and int(ids.max()) == 50256
    # the key is the seed's two halves, the counter the row's two halves, the unit and the purpose
    assert [int(x) for x in T.draw(0x299f31d0a4093822, 0x85a308d3243f6a88, 0x13198a2e, 0x03707344)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # a word's draw is not the draw of the column with that number, and B's words are not A's
    d = [int(T.draw(1234, 5, 9, purpose)[0]) for purpose in (T.COLUMN, T.WORD_A, T.WORD_B)]
    assert len(set(d)) == 3
    assert T.threshold(0.0) == 0 and T.threshold(1.0) == ONE and T.threshold(0.15) == 644245094


# ---- the rules on rows worked by hand -----------------------------------------------------------------------------------
def rows(*r):
    return np.array(r, dtype=np.int64)


PAD_RIGHT = dict(ids=rows([1, 10, 11, 12, 2, 0]), mask=rows([1, 1, 1, 1, 1, 0]), plan=rows([0, 0, 0, 3, 1, 0, 0, 4]))
PAD_LEFT = dict(ids=rows([0, 1, 10, 11, 12, 2]), mask=rows([0, 1, 1, 1, 1, 1]), plan=rows([0, 0, 0, 3, 2, 0, 0, 5]))
PAIR = dict(ids=rows([1, 10, 11, 3, 4, 20, 21, 22, 2, 0]), mask=rows([1] * 9 + [0]), plan=rows([0, 0, 0, 2, 1, 2, 3, 5]))
EMPTY_A = dict(ids=rows([1, 3, 4, 20, 2, 0]), mask=rows([1, 1, 1, 1, 1, 0]), plan=rows([0, 0, 0, 0, 1, 0, 1, 3]))
EMPTY_B = dict(ids=rows([1, 10, 3, 4, 2, 0]), mask=rows([1, 1, 1, 1, 1, 0]), plan=rows([0, 0, 0, 1, 1, 1, 0, 4]))


def mlm(case, **kw):
    out, labels, wrong = T.mlm_ref(case["ids"], case["plan"], **dict(ALWAYS, **kw))
    assert not wrong
    return out[0].tolist(), labels[0].tolist()


def lab(case, flags, wrong=False):
    labels, w = T.labels_ref(case["ids"], case["mask"], case["plan"], flags)
    assert w == wrong
    return labels[0].tolist()


def test_corruption_of_worked_rows():
    assert mlm(PAD_RIGHT) == ([1, M, M, M, 2, 0], [I, 10, 11, 12, I, I])
    assert mlm(PAD_LEFT) == ([0, 1, M, M, M, 2], [I, I, 10, 11, 12, I])
    assert mlm(PAIR) == ([1, M, M, 3, 4, M, M, M, 2, 0], [I, 10, 11, I, I, 20, 21, 22, I, I])
    assert mlm(PAIR, sides=T.SIDE_A) == ([1, M, M, 3, 4, 20, 21, 22, 2, 0], [I, 10, 11, I, I, I, I, I, I, I])
    assert mlm(PAIR, sides=T.SIDE_B) == ([1, 10, 11, 3, 4, M, M, M, 2, 0], [I, I, I, I, I, 20, 21, 22, I, I])
    assert mlm(EMPTY_A) == ([1, 3, 4, M, 2, 0], [I, I, I, 20, I, I])
    assert mlm(EMPTY_A, sides=T.SIDE_A) == ([1, 3, 4, 20, 2, 0], [I] * 6)
    assert mlm(EMPTY_B) == ([1, M, 3, 4, 2, 0], [I, 10, I, I, I, I])
    # nothing selected: nothing changes; selected and kept: only the labels tell; selected and random: an id below vocab
    assert mlm(PAIR, select_below=0) == (PAIR["ids"][0].tolist(), [I] * 10)
    assert mlm(PAIR, mask_below=0, random_below=0) == (PAIR["ids"][0].tolist(), [I, 10, 11, I, I, 20, 21, 22, I, I])
    out, labels = mlm(PAIR, mask_below=0, vocab_size=7)
    assert labels == [I, 10, 11, I, I, 20, 21, 22, I, I] and all(0 <= out[c] < 7 for c in (1, 2, 5, 6, 7))
    assert [out[c] for c in (0, 3, 4, 8, 9)] == [1, 3, 4, 2, 0]
    u2 = T.draw(7, 0, np.array([1, 2, 5, 6, 7]), T.COLUMN)[2]
    assert [out[c] for c in (1, 2, 5, 6, 7)] == [int(x) * 7 >> 32 for x in u2]


def test_whole_word_corruption_of_worked_rows():
    words = np.array([0, 0, 1, 0, 1, 1], dtype=np.int32)  # A: two tokens of word 0, one of word 1; B: 0, 1, 1
    pair = dict(PAIR, plan=rows([0, 0, 0, 3, 1, 3, 3, 5]), ids=rows([1, 10, 11, 12, 4, 20, 21, 22, 2, 0]))
    seed = next(s for s in range(100) if len({bool(T.draw(s, 0, w, p)[0] < ONE // 2) for w in (0, 1) for p in (1, 2)}) == 2)
    out, labels, wrong = T.mlm_ref(pair["ids"], pair["plan"], words, **dict(ALWAYS, seed=seed, select_below=ONE // 2))
    assert not wrong
    sel = [x != I for x in labels[0].tolist()]
    want = {(p, w): bool(T.draw(seed, 0, w, p)[0] < ONE // 2) for w in (0, 1) for p in (1, 2)}
    assert sel == [False, want[1, 0], want[1, 0], want[1, 1], False, want[2, 0], want[2, 1], want[2, 1], False, False]
    assert [x == M for x in out[0].tolist()] == sel
    # the same words from two arrays; a word below 0 protects its token; a word outside its array is not read
    again = T.mlm_ref(pair["ids"], rows([0, 0, 0, 3, 1, 0, 3, 5]), words[:3], words[3:], **dict(ALWAYS, seed=seed, select_below=ONE // 2))
    assert np.array_equal(again[0], out) and np.array_equal(again[1], labels) and not again[2]
    case = dict(ids=rows([1, 10, 11, 12, 2, 0]), plan=rows([0, 0, 2, 3, 1, 0, 0, 4]))
    out, labels, wrong = T.mlm_ref(case["ids"], case["plan"], np.array([0, 0, -1, 1], dtype=np.int32), **ALWAYS)
    assert wrong and out[0].tolist() == [1, 10, M, 12, 2, 0] and labels[0].tolist() == [I, I, 11, I, I, I]


def test_labels_of_worked_rows():
    A, B, TPL, END, SH = T.LABELS_A, T.LABELS_B, T.LABELS_TEMPLATE, T.LABELS_END, T.LABELS_SHIFT
    ALL = A | B | TPL | END
    assert lab(PAD_RIGHT, ALL) == [1, 10, 11, 12, 2, I]
    assert lab(PAD_RIGHT, ALL | SH) == [10, 11, 12, 2, I, I]
    assert lab(PAD_RIGHT, A) == [I, 10, 11, 12, I, I] and lab(PAD_RIGHT, A | SH) == [10, 11, 12, I, I, I]
    assert lab(PAD_RIGHT, TPL) == [1, I, I, I, I, I] and lab(PAD_RIGHT, END) == [I, I, I, I, 2, I]
    assert lab(PAD_RIGHT, B) == [I] * 6
    assert lab(PAD_LEFT, ALL) == [I, 1, 10, 11, 12, 2]
    assert lab(PAD_LEFT, ALL | SH) == [I, 10, 11, 12, 2, I]  # the last pad column predicts nothing, nor does the last column
    assert lab(PAIR, ALL) == [1, 10, 11, 3, 4, 20, 21, 22, 2, I]
    assert lab(PAIR, B | END) == [I, I, I, I, I, 20, 21, 22, 2, I]  # completion
    assert lab(PAIR, B | END | SH) == [I, I, I, I, 20, 21, 22, 2, I, I]
    assert lab(PAIR, TPL) == [1, I, I, 3, 4, I, I, I, I, I] and lab(PAIR, TPL | SH) == [I, I, 3, 4, I, I, I, I, I, I]
    assert lab(EMPTY_A, TPL) == [1, 3, 4, I, I, I] and lab(EMPTY_A, B | END) == [I, I, I, 20, 2, I]
    assert lab(EMPTY_B, TPL) == [1, I, 3, 4, I, I] and lab(EMPTY_B, A | END) == [I, 10, I, I, 2, I]
    # a row that fills its length: the last real column is L - 1
    full = dict(ids=rows([1, 10, 11, 2]), mask=rows([1, 1, 1, 1]), plan=rows([0, 0, 0, 2, 1, 0, 0, 3]))
    assert lab(full, ALL) == [1, 10, 11, 2] and lab(full, ALL | SH) == [10, 11, 2, I]


def test_hostile_plans_by_the_restatement():
    ids = rows([5, 6, 7, 8, 9, 10])
    mask = rows([1] * 6)
    # A begins in front of the row (clipped to columns 0, 1); B claims column 1 too (it is A's) and 2, 3
    plan = rows([0, 0, 0, 4, -2, 0, 3, 1])
    out, labels, wrong = T.mlm_ref(ids, plan, **ALWAYS)
    assert wrong and out[0].tolist() == [M, M, M, M, 9, 10]
    out, labels, wrong = T.mlm_ref(ids, plan, **dict(ALWAYS, sides=T.SIDE_B))
    assert wrong and out[0].tolist() == [5, 6, M, M, 9, 10] and labels[0].tolist() == [I, I, 7, 8, I, I]
    got, wrong = T.labels_ref(ids, mask, plan, T.LABELS_A)
    assert wrong and got[0].tolist() == [5, 6, I, I, I, I]
    got, wrong = T.labels_ref(ids, mask, plan, T.LABELS_END)  # col_b + kb = 4
    assert wrong and got[0].tolist() == [I, I, I, I, 9, 10]
    # negative lengths count as 0, sides beyond the row hold no column
    for plan in (rows([0, 0, 0, -3, 1, 0, -1, 2]), rows([0, 0, 0, 2, 6, 0, 2, 2**62]), rows([0, 0, 0, 2**63 - 1, -2**62, 0, 0, 0])):
        out, labels, wrong = T.mlm_ref(ids, plan, **ALWAYS)
        assert wrong and out[0].tolist() == ids[0].tolist() and (labels == I).all()
    assert T.clip_side(2, 2**63 - 1, 6) == (2, 6, True) and T.clip_side(0, 6, 6) == (0, 6, False)
    assert T.clip_side(5, 1, 6) == (5, 6, False) and T.clip_side(6, 1, 6) == (0, 0, True) and T.clip_side(3, 0, 6) == (0, 0, False)


# ---- the Python surface: argument checks come before any device call ------------------------------------------------
def test_names_are_exported():
    for name in ("mask_tokens", "lm_labels", "batch_encode_mlm"):
        assert name in hutoken_amd.__all__ and callable(getattr(hutoken_amd, name))
    for name in ("hutk_rows_mlm_device", "hutk_rows_labels_device"):
        assert name in _capi.EXPORTS
        assert hasattr(_capi.load(), name) and getattr(_capi.load(), name).argtypes is not None
    assert (_capi.MLM_SIDE_A, _capi.MLM_SIDE_B) == (T.SIDE_A, T.SIDE_B)
    assert (_capi.LABELS_A, _capi.LABELS_B, _capi.LABELS_TEMPLATE, _capi.LABELS_END, _capi.LABELS_SHIFT) == (1, 2, 4, 8, 16)


def host_rows(n=2, L=4, dtype=None):
    import torch
    return torch.zeros((n, L), dtype=dtype or torch.int32), torch.zeros((n, 8), dtype=torch.int64)


def test_mask_tokens_argument_checks():
    import torch
    ids, plan = host_rows()
    ok = dict(mask_id=3, seed=0, vocab_size=10)
    call = hutoken_amd.mask_tokens
    with pytest.raises(TypeError, match="seed"):
        call(ids, plan, mask_id=3)  # no default
    with pytest.raises(TypeError, match="mask_id"):
        call(ids, plan, seed=0)
    for bad in ([[1, 2]], None, np.zeros((2, 4), dtype=np.int32)):
        with pytest.raises(TypeError, match="input_ids"):
            call(bad, plan, **ok)
    for bad in (torch.int16, torch.float32, torch.uint8, torch.bool):
        with pytest.raises(TypeError, match="input_ids"):
            call(ids.to(bad), plan, **ok)
    for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 8), dtype=torch.int32)[:, ::2],
                torch.zeros((2, 2, 2), dtype=torch.int32)):
        with pytest.raises(ValueError, match="input_ids"):
            call(bad, plan, **ok)
    with pytest.raises(TypeError, match="row_plan"):
        call(ids, plan.to(torch.int32), **ok)
    for bad in (torch.zeros((3, 8), dtype=torch.int64), torch.zeros((2, 7), dtype=torch.int64)):
        with pytest.raises(ValueError, match="row_plan"):
            call(ids, bad, **ok)
    for name in ("mlm_probability", "mask_fraction", "random_fraction"):
        for bad in (-0.1, 1.5, float("nan"), 2):
            with pytest.raises(ValueError, match=name):
                call(ids, plan, **dict(ok, **{name: bad}))
        for bad in ("0.5", None, True):
            with pytest.raises(TypeError, match=name):
                call(ids, plan, **dict(ok, **{name: bad}))
    with pytest.raises(ValueError, match="mask_fraction \\+ random_fraction"):
        call(ids, plan, mask_fraction=0.8, random_fraction=0.3, **ok)
    for bad in (True, 1.0, "1", None):
        with pytest.raises(TypeError, match="seed"):
            call(ids, plan, mask_id=3, vocab_size=10, seed=bad)
    for bad in (-1, 2**64):
        with pytest.raises(ValueError, match="seed"):
            call(ids, plan, mask_id=3, vocab_size=10, seed=bad)
    with pytest.raises(ValueError, match="vocab_size=None"):
        call(ids, plan, mask_id=3, seed=0)
    with pytest.raises(ValueError, match="vocab_size=None"):
        call(ids, plan, mask_id=3, seed=0, random_fraction=0.05)
    for bad in (0, -5, 2**31 + 1):
        with pytest.raises(ValueError, match="vocab_size"):
            call(ids, plan, mask_id=3, seed=0, vocab_size=bad)
    for bad in (10.0, True, "10"):
        with pytest.raises(TypeError, match="vocab_size"):
            call(ids, plan, mask_id=3, seed=0, vocab_size=bad)
    for bad in (None, 1.0, True):
        with pytest.raises(TypeError, match="mask_id"):
            call(ids, plan, mask_id=bad, seed=0, vocab_size=10)
    with pytest.raises(ValueError, match="mask_id"):
        call(ids, plan, mask_id=2**31, seed=0, vocab_size=10)
    for bad in ("A", "ab", 3, None):
        with pytest.raises(ValueError, match="sides"):
            call(ids, plan, sides=bad, **ok)
    with pytest.raises(ValueError, match="fit int32"):
        call(ids, plan, ignore_index=2**31, **ok)
    with pytest.raises(ValueError, match="fit int64"):
        call(ids.to(torch.int64), plan, ignore_index=2**63, **ok)
    with pytest.raises(TypeError, match="ignore_index"):
        call(ids, plan, ignore_index=-100.0, **ok)
    with pytest.raises(TypeError, match="inplace"):
        call(ids, plan, inplace=1, **ok)
    words = torch.zeros(5, dtype=torch.int32)
    for bad in ([0, 1], np.zeros(5, dtype=np.int32)):
        with pytest.raises(TypeError, match="word_ids"):
            call(ids, plan, word_ids=bad, **ok)
    with pytest.raises(TypeError, match="word_ids"):
        call(ids, plan, word_ids=words.to(torch.int64), **ok)
    with pytest.raises(ValueError, match="word_ids"):
        call(ids, plan, word_ids=torch.zeros((5, 1), dtype=torch.int32), **ok)
    with pytest.raises(TypeError, match="word_ids_b"):
        call(ids, plan, word_ids=words, word_ids_b=words.to(torch.int16), **ok)
    with pytest.raises(ValueError, match="word_ids_b needs word_ids"):
        call(ids, plan, word_ids_b=words, **ok)
    # sound arguments on the host: refused for where they are, not computed there
    for kw in ({}, {"word_ids": words}, {"word_ids": words, "word_ids_b": words, "sides": "b"}, {"inplace": True},
               {"vocab_size": None, "random_fraction": 0, "mask_fraction": 1}, {"mlm_probability": 1, "seed": 2**64 - 1}):
        with pytest.raises(ValueError, match="on the GPU"):
            call(ids, plan, **dict(ok, **kw))
        with pytest.raises(ValueError, match="on the GPU"):
            call(ids.to(torch.int64), plan, **dict(ok, **kw))
    assert not ids.any()  # (inplace=True wrote nothing)


def test_lm_labels_argument_checks():
    import torch
    ids, plan = host_rows()
    mask = torch.ones((2, 4), dtype=torch.uint8)
    call = hutoken_amd.lm_labels
    for bad in ([[1, 2]], None):
        with pytest.raises(TypeError, match="input_ids"):
            call(bad, mask, plan)
    with pytest.raises(TypeError, match="input_ids"):
        call(ids.to(torch.float32), mask, plan)
    with pytest.raises(ValueError, match="input_ids"):
        call(torch.zeros(8, dtype=torch.int32), mask, plan)
    for bad in (None, [[1] * 4] * 2):
        with pytest.raises(TypeError, match="attention_mask"):
            call(ids, bad, plan)
    for bad in (torch.int32, torch.bool, torch.int8):
        with pytest.raises(TypeError, match="attention_mask"):
            call(ids, mask.to(bad), plan)
    for bad in (torch.ones((2, 5), dtype=torch.uint8), torch.ones(8, dtype=torch.uint8), torch.ones((2, 8), dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError, match="attention_mask"):
            call(ids, bad, plan)
    with pytest.raises(TypeError, match="row_plan"):
        call(ids, mask, None)
    with pytest.raises(ValueError, match="row_plan"):
        call(ids, mask, torch.zeros((1, 8), dtype=torch.int64))
    for bad in ("some", "ALL", (), ("a", "c"), ("a", 1), None, 5):
        with pytest.raises(ValueError, match="loss_on"):
            call(ids, mask, plan, loss_on=bad)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="shift"):
            call(ids, mask, plan, shift=bad)
    with pytest.raises(ValueError, match="fit int32"):
        call(ids, mask, plan, ignore_index=-2**31 - 1)
    with pytest.raises(TypeError, match="ignore_index"):
        call(ids, mask, plan, ignore_index=True)
    for kw in ({}, {"loss_on": "completion", "shift": True}, {"loss_on": ("b", "end")}, {"loss_on": ["template"], "ignore_index": 0}):
        with pytest.raises(ValueError, match="on the GPU"):
            call(ids, mask, plan, **kw)
    assert hutoken_amd._loss_on_arg("all") == 15 and hutoken_amd._loss_on_arg("completion") == 10
    assert hutoken_amd._loss_on_arg(("a", "template", "a")) == 5


def test_batch_encode_mlm_checks_before_it_encodes(monkeypatch):
    call = hutoken_amd.batch_encode_mlm
    monkeypatch.setattr(hutoken_amd, "_ctx", None)
    with pytest.raises(TypeError, match="seed"):
        call(["a"], 8, mask_id=3)
    with pytest.raises(TypeError, match="whole_word"):
        call(["a"], 8, mask_id=3, seed=0, vocab_size=10, whole_word=1)
    with pytest.raises(TypeError, match="plan"):
        call(["a"], 8, mask_id=3, seed=0, vocab_size=10, return_plan=True)
    with pytest.raises(ValueError, match="vocab_size=None"):
        call(["a"], 8, mask_id=3, seed=0)
    with pytest.raises(ValueError, match="mlm_probability"):
        call(["a"], 8, mask_id=3, seed=0, vocab_size=10, mlm_probability=2.0)
    with pytest.raises(RuntimeError, match="initialize"):
        call(["a"], 8, mask_id=3, seed=0, vocab_size=10)

    class NoPreset:  # a context with the built-in splitter: nothing is encoded before whole words are refused
        pretokenizer = None
    monkeypatch.setattr(hutoken_amd, "_ctx", NoPreset())
    with pytest.raises(ValueError, match="split preset"):
        call(["a"], 8, mask_id=3, seed=0, vocab_size=10, whole_word=True)


# ---- the C ABI: what is refused before a device is looked for -------------------------------------------------------
def c_mlm(n_rows=0, max_len=8, width=4, n_a=0, n_b=0, select=0, mask=0, random=0, vocab=1, ignore=-100, sides=3, plan=None,
          ids=None, words_a=None, words_b=None, out=None, labels=None, err=None):
    return _capi.load().hutk_rows_mlm_device(plan, n_rows, max_len, ids, width, words_a, n_a, words_b, n_b, 1234, select, mask,
                                             random, 7, vocab, ignore, sides, out, labels, err, None)


def c_labels(n_rows=0, max_len=8, width=4, flags=15, ignore=-100, plan=None, ids=None, mask=None, labels=None, err=None):
    return _capi.load().hutk_rows_labels_device(plan, n_rows, max_len, ids, width, mask, flags, ignore, labels, err, None)


def test_c_abi_argument_checks_need_no_device():
    E = _capi.E_ARG
    for call in (c_mlm, c_labels):
        for width in (0, 2, 16, -4):
            assert call(width=width) == E
        for max_len in (0, -1, 2**31):
            assert call(max_len=max_len) == E
        assert call(n_rows=-1) == E
        assert call(ignore=2**31) == E and call(ignore=-2**31 - 1) == E  # does not fit int32 rows
        assert "ignore_index" in _capi.last_error()
        # with rows: a NULL buffer, a misaligned one, labels that are an input (addresses that nothing reads: refused first)
        assert call(n_rows=1) == E and "NULL" in _capi.last_error()
        assert call(n_rows=1, plan=0x1000, ids=0x2002, labels=0x4000, **({"out": 0x3000} if call is c_mlm else {"mask": 0x3000})) == E
        assert "aligned" in _capi.last_error()
        assert call(n_rows=1, plan=0x1004, ids=0x2000, labels=0x4000, **({"out": 0x3000} if call is c_mlm else {"mask": 0x3000})) == E
        assert call(n_rows=1, plan=0x1000, ids=0x2000, labels=0x2000, **({"out": 0x3000} if call is c_mlm else {"mask": 0x3000})) == E
        assert "overlap" in _capi.last_error()
        assert call(n_rows=2, plan=0x1000, ids=0x2000, labels=0x2020, **({"out": 0x3000} if call is c_mlm else {"mask": 0x3000})) == E
        assert call(n_rows=1, width=8, plan=0x1000, ids=0x2004, labels=0x4000, **({"out": 0x3000} if call is c_mlm else {"mask": 0x3000})) == E
        assert call(err=0x1002) == E
    assert c_mlm(words_a=0x1000, n_a=-1) == E and c_mlm(words_a=0x1000, n_b=-1) == E
    for kw in (dict(select=-1), dict(select=2**32 + 1), dict(mask=-1), dict(mask=2, random=1), dict(random=2**32 + 1),
               dict(mask=2**32 + 1, random=2**32 + 1)):
        assert c_mlm(**kw) == E, kw
    assert "thresholds" in _capi.last_error()
    for vocab in (0, -1, 2**31 + 1):
        assert c_mlm(vocab=vocab) == E
    for sides in (0, 4, 7, -1):
        assert c_mlm(sides=sides) == E
    assert c_mlm(n_rows=1, plan=0x1000, ids=0x2000, out=0x2010, labels=0x4000) == E  # out is neither ids nor apart from it
    assert c_mlm(n_rows=1, plan=0x1000, ids=0x2000, out=0x3000, labels=0x3000) == E  # labels are the other output
    assert c_mlm(n_rows=1, plan=0x1000, ids=0x2000, out=0x2000, labels=0x4000, words_a=0x5002) == E  # misaligned word ids
    assert c_mlm(n_rows=1, plan=0x1000, ids=0x2000, out=0x2000, labels=0x2008, max_len=4) == E  # inplace; labels inside the row
    for flags in (0, 16, 32, 47, -1):
        assert c_labels(flags=flags) == E
    assert "flags" in _capi.last_error()
    assert c_labels(n_rows=1, plan=0x1000, ids=0x2000, mask=0x4004, labels=0x4000) == E  # labels over the mask
    assert c_labels(n_rows=1, width=8, ignore=2**40, plan=0x1000, ids=0x2000, mask=None, labels=0x4000) == E  # no mask


def test_sound_arguments_without_rows():
    """Limits that are allowed, with n_rows == 0: nothing is written and nothing launched; without a GPU the calls fail
    loudly after the argument checks."""
    import torch
    want = _capi.OK if torch.cuda.is_available() else _capi.E_DEVICE
    assert c_mlm(select=2**32, mask=2**32, random=2**32, vocab=2**31, sides=1) == want
    assert c_mlm(width=8, ignore=2**62, max_len=2**31 - 1, words_a=0x1000, n_a=5, sides=2) == want
    assert c_labels(flags=31, width=8, ignore=-2**63) == want and c_labels(flags=8, max_len=1) == want
