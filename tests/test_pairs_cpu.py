"""Pair collation without a GPU: the NumPy reference (tests/pairs_ref.py) against the worked examples typed out by hand and
-- where the `tokenizers` package is installed -- against its pair truncation and overflowing rows, the vectorised forms
against the loop forms, the rows bound, the exports, and the argument checks of the Python surface and the C ABI, which
run before any device call."""
import random

import numpy as np
import pytest

import hutoken_amd
import pairs_ref as R
from hutoken_amd import _capi

NO = _capi.NO_TOKEN
LONGEST_FIRST, ONLY_FIRST, ONLY_SECOND = 0, 1, 2  # HUTK_PAIR_* (test_names_are_exported pins _capi's to them)


# ---- the reference itself, pinned by hand -------------------------------------------------------------------------
def test_worked_kept_lengths():
    assert R.pair_lengths(4, 4, 5, "longest_first") == (2, 3)  # a tie: B gets the odd id
    assert R.pair_lengths(5, 4, 5, "longest_first") == (3, 2)  # the longer side gets it
    assert R.pair_lengths(2, 9, 7, "longest_first") == (2, 5)
    assert R.pair_lengths(12, 9, 7, "longest_first") == (4, 3)
    assert R.pair_lengths(9, 12, 7, "longest_first") == (3, 4)
    assert R.pair_lengths(3, 4, 7, "longest_first") == (3, 4)  # they fit: nothing is cut, under every strategy
    assert R.pair_lengths(3, 4, 7, "only_first") == (3, 4) and R.pair_lengths(3, 4, 7, "only_second") == (3, 4)
    assert R.pair_lengths(6, 4, 7, "only_first") == (3, 4)
    assert R.pair_lengths(6, 9, 7, "only_first") == (0, 7)   # the side not named is cut when it alone exceeds R
    assert R.pair_lengths(6, 4, 7, "only_second") == (6, 1)
    assert R.pair_lengths(9, 4, 7, "only_second") == (7, 0)
    assert R.pair_lengths(0, 0, 1, "longest_first") == (0, 0)
    assert R.pair_lengths(0, 3, 1, "longest_first") == (0, 1) and R.pair_lengths(3, 0, 1, "longest_first") == (1, 0)
    assert R.pair_lengths(3, 3, 1, "longest_first") == (0, 1)


def test_worked_rows():
    a, oa = R.ragged([[10, 11, 12, 13], [20, 21, 22, 23, 24], []])
    b, ob = R.ragged([[50, 51, 52, 53], [60, 61, 62, 63], [-70]])
    out, mask, types, lengths = R.pairs(a, oa, b, ob, 8, bos_id=1, sep_ids=(4,), eos_id=2, pad_id=0)  # R = 5
    assert out.tolist() == [[1, 10, 11, 4, 50, 51, 52, 2], [1, 20, 21, 22, 4, 60, 61, 2], [1, 4, -70, 2, 0, 0, 0, 0]]
    assert mask.tolist() == [[1] * 8, [1] * 8, [1, 1, 1, 1, 0, 0, 0, 0]]
    assert types.tolist() == [[0, 0, 0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 0, 0, 0, 0]]
    assert lengths.tolist() == [8, 8, 4] and lengths.dtype == np.int32 and types.dtype == np.uint8
    out, mask, types, lengths = R.pairs(a, oa, b, ob, 8, "only_first", sep_ids=(4, 4), eos_id=2, pad_id=-1,
                                        padding_side="left", dtype=np.int64)  # RoBERTa's two separators, no bos: R = 5
    assert out.dtype == np.int64
    assert out.tolist() == [[10, 4, 4, 50, 51, 52, 53, 2], [20, 4, 4, 60, 61, 62, 63, 2], [-1, -1, -1, -1, 4, 4, -70, 2]]
    assert mask.tolist() == [[1] * 8, [1] * 8, [0, 0, 0, 0, 1, 1, 1, 1]]
    assert types.tolist() == [[0, 0, 0, 1, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 1, 1]]
    assert lengths.tolist() == [8, 8, 4]
    out, _mask, types, lengths = R.pairs(a, oa, b, ob, 4, "only_second")  # nothing but the ids: R = 4
    assert out.tolist() == [[10, 11, 12, 13], [20, 21, 22, 23], [-70, 0, 0, 0]]
    assert types.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]] and lengths.tolist() == [4, 4, 1]


def test_worked_windows():
    a, oa = R.ragged([[100, 101, 102]])
    b, ob = R.ragged([list(range(200, 212))])
    kw = dict(bos_id=1, sep_ids=(4,), eos_id=2)
    out, mask, types, lengths, row_map = R.pair_windows(a, oa, b, ob, 10, 2, "only_second", **kw)  # R = 7, C = 4, step = 2
    head = [1, 100, 101, 102, 4]
    assert out.tolist() == [head + [200, 201, 202, 203, 2], head + [202, 203, 204, 205, 2], head + [204, 205, 206, 207, 2],
                            head + [206, 207, 208, 209, 2], head + [208, 209, 210, 211, 2]]
    assert mask.tolist() == [[1] * 10] * 5 and types.tolist() == [[0] * 5 + [1] * 5] * 5
    assert lengths.tolist() == [10] * 5 and row_map.tolist() == [[0, 0], [0, 2], [0, 4], [0, 6], [0, 8]]
    assert R.row_offsets(oa, ob, 10, 2, "only_second", **kw).tolist() == [0, 5]
    # the same pair the other way round: A is cut, B kept whole; and a last window that is the short one
    out, mask, types, lengths, row_map = R.pair_windows(b, ob, a, oa, 10, 1, "only_first", **kw)  # C = 4, step = 3
    tail = [4, 100, 101, 102, 2]
    assert out.tolist() == [[1, 200, 201, 202, 203] + tail, [1, 203, 204, 205, 206] + tail, [1, 206, 207, 208, 209] + tail,
                            [1, 209, 210, 211] + tail + [0]]
    assert types.tolist() == [[0] * 6 + [1] * 4] * 3 + [[0] * 5 + [1] * 4 + [0]]
    assert mask.tolist() == [[1] * 10] * 3 + [[1] * 9 + [0]] and lengths.tolist() == [10, 10, 10, 9]
    assert row_map.tolist() == [[0, 0], [0, 3], [0, 6], [0, 9]]
    # a kept side that fills the row: C == 0, one row, the cut side empty; and one that leaves C <= stride: step 1
    a, oa = R.ragged([list(range(10, 20)), [10, 11, 12, 13, 14]])
    b, ob = R.ragged([[50, 51], [50, 51, 52, 53]])
    out, _mask, types, lengths, row_map = R.pair_windows(a, oa, b, ob, 8, 4, "only_second", sep_ids=(4,))  # R = 7
    assert out.tolist() == [[10, 11, 12, 13, 14, 15, 16, 4], [10, 11, 12, 13, 14, 4, 50, 51], [10, 11, 12, 13, 14, 4, 51, 52],
                            [10, 11, 12, 13, 14, 4, 52, 53]]
    assert types.tolist() == [[0] * 8] + [[0] * 6 + [1, 1]] * 3
    assert lengths.tolist() == [8] * 4 and row_map.tolist() == [[0, 0], [1, 0], [1, 1], [1, 2]]
    empty = R.pair_windows(*R.ragged([]), *R.ragged([]), 4)
    assert [x.shape for x in empty] == [(0, 4), (0, 4), (0, 4), (0,), (0, 2)]
    assert [x.shape for x in R.pair_windows_vec(*R.ragged([]), *R.ragged([]), 4)] == [(0, 4), (0, 4), (0, 4), (0,), (0, 2)]
    assert [x.shape for x in R.pairs_vec(*R.ragged([]), *R.ragged([]), 4)] == [(0, 4), (0, 4), (0, 4), (0,)]


def same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


def test_vectorised_forms_equal_the_loop_forms():
    rnd = random.Random(5)
    for trial in range(200):
        n = rnd.randrange(0, 9)
        lens = (0, 1, 2, 3, 5, 8, 13, 40)
        docs_a = [[rnd.randrange(-3, 1000) for _ in range(rnd.choice(lens))] for _ in range(n)]
        docs_b = [[rnd.randrange(-3, 1000) for _ in range(rnd.choice(lens))] for _ in range(n)]
        a, oa = R.ragged(docs_a, base=rnd.choice((0, 0, 3)), tail=rnd.choice((0, 2)))
        b, ob = R.ragged(docs_b, base=rnd.choice((0, 1, 7)))
        if trial % 4 == 0:  # both sides in one ids array, B's offsets a view with a non-zero base
            a, oo = R.ragged(docs_a + docs_b, base=rnd.choice((0, 2)))
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
            for dtype in (np.int32, np.int64):
                for strategy in R.STRATEGIES:
                    label = (trial, docs_a, docs_b, L, stride, kw, side, strategy)
                    x = R.pairs(a, oa, b, ob, L, strategy, pad_id=-7, padding_side=side, dtype=dtype, **kw)
                    y = R.pairs_vec(a, oa, b, ob, L, strategy, pad_id=-7, padding_side=side, dtype=dtype, **kw)
                    assert len(x) == len(y) == 4 and all(same(p, q) for p, q in zip(x, y)), label
                    if strategy == "longest_first":
                        continue
                    x = R.pair_windows(a, oa, b, ob, L, stride, strategy, pad_id=-7, padding_side=side, dtype=dtype, **kw)
                    y = R.pair_windows_vec(a, oa, b, ob, L, stride, strategy, pad_id=-7, padding_side=side, dtype=dtype, **kw)
                    assert len(x) == len(y) == 5 and all(same(p, q) for p, q in zip(x, y)), label
                    ro = R.row_offsets(oa, ob, L, stride, strategy, **kw)
                    assert np.array_equal(ro, R.row_table(oa, ob, L, stride, strategy, **kw)[0]) and ro[-1] == len(x[0])
                    # the first window of every pair is the one-row form's row
                    one = R.pairs(a, oa, b, ob, L, strategy, pad_id=-7, padding_side=side, dtype=dtype, **kw)
                    assert all(same(p[ro[:-1]], q) for p, q in zip(x[:4], one)), label


def test_kept_lengths_hold_their_invariants():
    for strategy in R.STRATEGIES:
        for Rm in range(1, 12):
            for na in range(0, 30):
                for nb in range(0, 30):
                    ka, kb = R.pair_lengths(na, nb, Rm, strategy)
                    assert 0 <= ka <= na and 0 <= kb <= nb and ka + kb == min(Rm, na + nb), (strategy, Rm, na, nb)
                    va, vb = R.pair_lengths_vec([na], [nb], Rm, strategy)
                    assert (int(va[0]), int(vb[0])) == (ka, kb)
                    if strategy == "longest_first" and na + nb > Rm:
                        assert abs(ka - kb) <= 1 or ka == na or kb == nb


def test_rows_never_exceed_the_bound():
    rnd = random.Random(11)
    for s in range(0, 7):
        kw = {"bos_id": 0} if s in (1, 3, 5, 6) else {}
        if s == 6:
            kw["eos_id"] = 1
        kw["sep_ids"] = tuple(range(s - len(kw)))
        for L in range(s + 1, s + 9):
            for stride in range(0, L - s):
                la = [rnd.randrange(0, 12) for _ in range(6)] + [0, L - s, L - s + 1, 0]
                lb = [rnd.randrange(0, 60) for _ in range(6)] + [0, 0, 40, L - s + 1]
                oa = np.concatenate([[0], np.cumsum(la)]).astype(np.int64)
                ob = np.concatenate([[0], np.cumsum(lb)]).astype(np.int64)
                for strategy in ("only_first", "only_second"):
                    n_rows = int(R.row_offsets(oa, ob, L, stride, strategy, **kw)[-1])
                    cut = int(ob[-1] if strategy == "only_second" else oa[-1])
                    bound = _capi.pair_rows_bound(len(la), cut, L, stride, s)
                    assert bound == R.rows_bound(len(la), cut)
                    assert len(la) <= n_rows <= bound, (s, L, stride, strategy)
                for n in range(0, 30):  # one pair of every length against every kept side
                    for no in range(0, L - s + 2):
                        assert R.window_count(n, no, L - s, stride) <= 1 + n


# ---- against tokenizers -------------------------------------------------------------------------------------------
WORDS_A = ["a%d" % i for i in range(16)]
WORDS_B = ["b%d" % i for i in range(16)]


def make_tokenizer():
    tk = pytest.importorskip("tokenizers")
    from tokenizers import models, pre_tokenizers, processors
    vocab = {w: 100 + i for i, w in enumerate(WORDS_A)}
    vocab.update({w: 200 + i for i, w in enumerate(WORDS_B)})
    vocab.update({"[BOS]": 1, "[EOS]": 2, "[UNK]": 3, "[SEP]": 4})
    tok = tk.Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tok.post_processor = processors.TemplateProcessing(single="[BOS] $A [EOS]", pair="[BOS] $A:0 [SEP]:0 $B:1 [EOS]:1",
                                                       special_tokens=[("[BOS]", 1), ("[SEP]", 4), ("[EOS]", 2)])
    return tok


TEMPLATE = dict(bos_id=1, sep_ids=(4,), eos_id=2)


def our_rows(fn, na, nb, L, *args):
    a, oa = R.ragged([list(range(100, 100 + na))])
    b, ob = R.ragged([list(range(200, 200 + nb))])
    res = fn(a, oa, b, ob, L, *args, **TEMPLATE)
    return [(row[:m].tolist(), t[:m].tolist()) for row, t, m in zip(res[0], res[2], res[3])]


def test_kept_lengths_equal_tokenizers_pair_truncation():
    tok = make_tokenizer()
    compared = raised = 0
    for strategy in R.STRATEGIES:
        for L in range(4, 14):
            tok.enable_truncation(max_length=L, stride=0, strategy=strategy)
            Rm = L - 3
            for na in range(16):
                for nb in range(16):
                    ka, kb = R.pair_lengths(na, nb, Rm, strategy)
                    try:
                        enc = tok.encode(" ".join(WORDS_A[:na]), " ".join(WORDS_B[:nb]))
                    except Exception:
                        # tokenizers refuses to cut a side to nothing, and to cut the side that is not named
                        raised += 1
                        assert ka == 0 or kb == 0 or (strategy == "only_first" and nb > Rm - ka) or \
                            (strategy == "only_second" and na > Rm - kb), (strategy, L, na, nb)
                        continue
                    assert [(enc.ids, enc.type_ids)] == our_rows(R.pairs, na, nb, L, strategy), (strategy, L, na, nb)
                    compared += 1
    assert (compared, raised) == (4340, 3340)


def test_windows_equal_tokenizers_overflowing_rows():
    tok = make_tokenizer()
    compared = 0
    for strategy in ("only_first", "only_second"):
        for L in range(4, 14):
            Rm = L - 3
            for na in range(16):
                for nb in range(16):
                    n, no = (nb, na) if strategy == "only_second" else (na, nb)
                    _ko, C, _step = R.window_sizes(no, Rm, 0)
                    if no > Rm:
                        continue  # tokenizers raises: the side that is not named would have to be cut
                    for stride in range(0, C):  # (none with C == 0, where tokenizers raises as well)
                        tok.enable_truncation(max_length=L, stride=stride, strategy=strategy)
                        enc = tok.encode(" ".join(WORDS_A[:na]), " ".join(WORDS_B[:nb]))
                        theirs = [(e.ids, e.type_ids) for e in [enc] + list(enc.overflowing)]
                        assert theirs == our_rows(R.pair_windows, na, nb, L, stride, strategy), (strategy, L, na, nb, stride)
                        compared += 1
    # per strategy and R = 1 .. 10: the kept side's 0 .. R - 1 ids leave C = R .. 1, each with C strides and the cut side's
    # 16 lengths: 16 * sum(R * (R + 1) / 2) = 16 * 220
    assert compared == 7040


# ---- the Python surface: argument checks come before any device call ----------------------------------------------
C_NAMES = ("hutk_pair_rows_bound", "hutk_pair_rows_device", "hutk_collate_pairs_device")
PY_NAMES = ("collate_pairs", "collate_pair_windows", "batch_encode_pairs", "batch_encode_pair_windows")


def test_names_are_exported():
    for name in PY_NAMES:
        assert name in hutoken_amd.__all__ and callable(getattr(hutoken_amd, name))
    for name in C_NAMES:
        assert name in _capi.EXPORTS
        assert hasattr(_capi.load(), name)
    assert (_capi.PAIR_LONGEST_FIRST, _capi.PAIR_ONLY_FIRST, _capi.PAIR_ONLY_SECOND) == (0, 1, 2)


def host_pairs():
    import torch
    return (torch.tensor([1, 2, 3], dtype=torch.int32), torch.tensor([0, 1, 3], dtype=torch.int64),
            torch.tensor([4, 5], dtype=torch.int32), torch.tensor([0, 2, 2], dtype=torch.int64))


@pytest.mark.parametrize("windows", [False, True])
def test_python_argument_checks(windows):
    import torch
    a, oa, b, ob = host_pairs()
    fn = hutoken_amd.collate_pair_windows if windows else hutoken_amd.collate_pairs
    with pytest.raises(ValueError, match="on the GPU"):  # host tensors: there is no CPU path
        fn(a, oa, b, ob, 4)
    with pytest.raises(TypeError, match="torch tensor"):
        fn([1, 2, 3], oa, b, ob, 4)
    with pytest.raises(TypeError, match="torch tensor"):
        fn(a, oa, b, np.array([0, 2, 2]), 4)
    with pytest.raises(TypeError, match="int32"):
        fn(a, oa, b.long(), ob, 4)
    with pytest.raises(TypeError, match="int64"):
        fn(a, oa.int(), b, ob, 4)
    with pytest.raises(ValueError, match="one-dimensional"):
        fn(a.reshape(1, 3), oa, b, ob, 4)
    with pytest.raises(ValueError, match="as many documents"):
        fn(a, oa, b, ob[:2], 4)
    for bad in (0, -1, 2**31):
        with pytest.raises(ValueError, match="max_length"):
            fn(a, oa, b, ob, bad)
    with pytest.raises(ValueError, match="max_length"):  # max_length < s + 1: no room for a document id
        fn(a, oa, b, ob, 3, bos_id=1, sep_ids=(4,), eos_id=2)
    with pytest.raises(ValueError, match="max_length"):
        fn(a, oa, b, ob, 4, sep_ids=(4, 4, 4, 4))
    for bad in (2.0, "8", True):
        with pytest.raises(TypeError, match="max_length"):
            fn(a, oa, b, ob, bad)
    for bad in ("longest", "right", None, 1):
        with pytest.raises(ValueError, match="truncation"):
            fn(a, oa, b, ob, 4, truncation=bad)
    for bad in (4, "4", None, {4}):
        with pytest.raises(TypeError, match="sep_ids"):
            fn(a, oa, b, ob, 8, sep_ids=bad)
    with pytest.raises(ValueError, match="sep_ids"):
        fn(a, oa, b, ob, 8, sep_ids=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="sep_ids"):  # the C ABI's "absent" value
        fn(a, oa, b, ob, 8, sep_ids=[-2**31])
    with pytest.raises(ValueError, match="sep_ids"):
        fn(a, oa, b, ob, 8, sep_ids=(2**31,))
    with pytest.raises(TypeError, match="sep_ids"):
        fn(a, oa, b, ob, 8, sep_ids=(None,))
    with pytest.raises(ValueError, match="padding_side"):
        fn(a, oa, b, ob, 4, padding_side="both")
    for bad in (torch.float32, torch.int16, "int8", np.int32):
        with pytest.raises(ValueError, match="dtype"):
            fn(a, oa, b, ob, 4, dtype=bad)
    with pytest.raises(TypeError, match="bos_id"):
        fn(a, oa, b, ob, 4, bos_id="1")
    with pytest.raises(TypeError, match="pad_id"):
        fn(a, oa, b, ob, 4, pad_id=None)
    with pytest.raises(ValueError, match="eos_id"):
        fn(a, oa, b, ob, 4, eos_id=-2**31)
    with pytest.raises(TypeError):  # the options are keyword-only
        fn(a, oa, b, ob, 4, 0, "only_first") if windows else fn(a, oa, b, ob, 4, "only_first")


def test_python_argument_checks_of_the_windows_form():
    a, oa, b, ob = host_pairs()
    fn = hutoken_amd.collate_pair_windows
    with pytest.raises(ValueError, match="cross product"):  # the message says why
        fn(a, oa, b, ob, 8, truncation="longest_first")
    with pytest.raises(TypeError):  # max_length is required
        fn(a, oa, b, ob)
    with pytest.raises(TypeError, match="max_length"):
        fn(a, oa, b, ob, None)
    for L, stride, kw in ((4, -1, {}), (4, 4, {}), (4, 5, {}), (4, 3, {"eos_id": 2}), (6, 3, {"bos_id": 1, "sep_ids": (4,), "eos_id": 2}),
                          (1, 1, {})):
        with pytest.raises(ValueError, match="stride"):  # stride must stay below R = max_length - s
            fn(a, oa, b, ob, L, stride, **kw)
    for bad in (None, 1.0, "1", True):
        with pytest.raises(TypeError, match="stride"):
            fn(a, oa, b, ob, 4, bad)
    with pytest.raises(TypeError, match="n_rows"):
        fn(a, oa, b, ob, 4, n_rows=2.0)
    with pytest.raises(ValueError, match="n_rows"):
        fn(a, oa, b, ob, 4, n_rows=-1)
    with pytest.raises(TypeError):  # collate_pairs has neither stride nor n_rows
        hutoken_amd.collate_pairs(a, oa, b, ob, 4, n_rows=2)


def test_list_forms_check_their_texts(monkeypatch):
    monkeypatch.setattr(hutoken_amd, "_ctx", None)
    with pytest.raises(RuntimeError, match="not initialized"):
        hutoken_amd.batch_encode_pairs(["a"], ["b"], 8)
    with pytest.raises(RuntimeError, match="not initialized"):
        hutoken_amd.batch_encode_pair_windows(["a"], ["b"], 8, 2)
    monkeypatch.setattr(hutoken_amd, "_ctx", object())
    with pytest.raises(ValueError, match="as many texts"):
        hutoken_amd.batch_encode_pairs(["a", "b"], ["c"], 8)
    with pytest.raises(ValueError, match="as many texts"):
        hutoken_amd.batch_encode_pair_windows(["a"], [], 8)
    with pytest.raises(TypeError, match="lists"):
        hutoken_amd.batch_encode_pairs("a", ["c"], 8)
    with pytest.raises(ValueError):
        hutoken_amd.batch_encode_pairs(["a"], ["c"], 8, normalize="nfc-ish")


# ---- the C ABI: argument errors come before the device is looked for -----------------------------------------------
def rows_call(max_len, stride=0, strategy=ONLY_SECOND, bos=NO, sep=(), eos=NO, n_pairs=0, cap_a=0, cap_b=0):
    return _capi.pair_rows_device(0, 0, n_pairs, cap_a, cap_b, max_len, stride, strategy, bos, sep, eos, 0)


def fill_call(max_len, stride=0, strategy=LONGEST_FIRST, bos=NO, sep=(), eos=NO, flags=0, out_width=4, n_pairs=0,
              cap_a=0, cap_b=0, n_rows=0, row_offsets=0):
    return _capi.collate_pairs_device(0, 0, 0, 0, row_offsets, n_pairs, cap_a, cap_b, n_rows, max_len, stride, strategy, bos,
                                      sep, eos, 0, flags, out_width, 0)


def test_c_abi_argument_checks_need_no_device():
    for max_len, bos, sep, eos in ((0, NO, (), NO), (-3, NO, (), NO), (1, NO, (), 2), (3, 1, (4,), 2), (4, NO, (4, 4, 4, 4), NO),
                                   (2**31, 1, (), 2)):
        with pytest.raises(TypeError, match="max_len"):
            rows_call(max_len, 0, bos=bos, sep=sep, eos=eos)
        with pytest.raises(TypeError, match="max_len"):
            fill_call(max_len, 0, bos=bos, sep=sep, eos=eos)
        with pytest.raises(TypeError, match="max_len"):
            _capi.pair_rows_bound(1, 1, max_len, 0, (bos != NO) + len(sep) + (eos != NO))
    for max_len, stride, bos, sep, eos in ((4, -1, NO, (), NO), (4, 4, NO, (), NO), (4, 3, NO, (), 2), (6, 3, 1, (4,), 2),
                                           (1, 1, NO, (), NO)):
        with pytest.raises(TypeError, match="stride"):
            rows_call(max_len, stride, bos=bos, sep=sep, eos=eos)
        with pytest.raises(TypeError, match="stride"):
            fill_call(max_len, stride, bos=bos, sep=sep, eos=eos)
        with pytest.raises(TypeError, match="stride"):
            _capi.pair_rows_bound(1, 1, max_len, stride, (bos != NO) + len(sep) + (eos != NO))
    lib = _capi.load()
    assert lib.hutk_pair_rows_bound(1, 1, 4, 4, 0) < 0  # the C function itself: a negative error
    assert lib.hutk_pair_rows_bound(-1, 1, 4, 0, 0) < 0
    assert lib.hutk_pair_rows_bound(1, -1, 4, 0, 0) < 0
    assert lib.hutk_pair_rows_bound(1, 1, 9, 0, 7) < 0
    assert _capi.pair_rows_bound(3, 10, 8, 1, 6) == 13 and _capi.pair_rows_bound(0, 0, 1, 0, 0) == 0
    for bad in (-1, 3):
        with pytest.raises(TypeError, match="strategy"):
            rows_call(8, strategy=bad)
        with pytest.raises(TypeError, match="strategy"):
            fill_call(8, strategy=bad)
    with pytest.raises(TypeError, match="cut into windows"):  # the windows form wants a named side
        rows_call(8, strategy=_capi.PAIR_LONGEST_FIRST)
    with pytest.raises(TypeError, match="cut into windows"):
        fill_call(8, strategy=_capi.PAIR_LONGEST_FIRST, row_offsets=256)
    with pytest.raises(TypeError, match="sep_ids"):
        rows_call(8, sep=(1, 2, 3, 4, 5))
    with pytest.raises(TypeError, match="sep_ids"):
        fill_call(8, sep=(1, NO))
    assert lib.hutk_pair_rows_device(None, None, 0, 0, 0, 8, 0, 2, NO, None, 1, NO, None, None, None) == _capi.E_ARG
    assert lib.hutk_pair_rows_device(None, None, 0, 0, 0, 8, 0, 2, NO, None, -1, NO, None, None, None) == _capi.E_ARG
    with pytest.raises(TypeError, match="bad arguments"):
        fill_call(4, out_width=5)
    with pytest.raises(TypeError, match="bad arguments"):
        fill_call(4, flags=4)  # an unknown bit
    with pytest.raises(TypeError, match="HUTK_COLLATE_PAD_LEFT"):
        fill_call(4, flags=_capi.COLLATE_TRUNC_LEFT)  # pairs are cut on the right only
    for kw in ({"n_pairs": -1, "n_rows": -1}, {"cap_a": -1}, {"cap_b": -1}, {"n_rows": -1}):
        with pytest.raises(TypeError, match="bad arguments"):
            fill_call(4, **kw)
    with pytest.raises(TypeError, match="n_rows must be n_pairs"):  # one row per pair
        fill_call(4, n_pairs=2, n_rows=3)
    for kw in ({"n_pairs": -1}, {"cap_a": -1}, {"cap_b": -1}):
        with pytest.raises(TypeError, match="bad arguments"):
            rows_call(4, **kw)


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        rows_call(8, 1, bos=1, sep=(4,), eos=2)
    with pytest.raises(RuntimeError, match="no HIP device"):
        fill_call(8, 1, flags=_capi.COLLATE_PAD_LEFT)
    with pytest.raises(RuntimeError, match="no HIP device"):
        fill_call(8, 1, strategy=_capi.PAIR_ONLY_FIRST, row_offsets=256, n_rows=3)
