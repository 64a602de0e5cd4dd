"""Window collation without a GPU: the NumPy reference (tests/windows_ref.py) against the worked examples typed out by
hand and -- where the `tokenizers` package is installed -- against its overflowing rows, the vectorised form against the
loop form, the rows bound, and the argument checks of the Python surface and the C ABI, which run before any device call."""
import random

import numpy as np
import pytest

import hutoken_amd
import windows_ref as R
from hutoken_amd import _capi

NO = _capi.NO_TOKEN


# ---- the reference itself, pinned by hand -----------------------------------------------------------------------
def test_worked_examples():
    kw = dict(bos_id=1, eos_id=2, pad_id=0)  # L = 6, stride = 1: C = 4, step = 3
    out, mask, lengths, row_map = R.windows(*R.ragged([list(range(10, 20))]), 6, 1, **kw)
    assert out.tolist() == [[1, 10, 11, 12, 13, 2], [1, 13, 14, 15, 16, 2], [1, 16, 17, 18, 19, 2]]
    assert mask.tolist() == [[1] * 6] * 3 and lengths.tolist() == [6, 6, 6]
    assert row_map.tolist() == [[0, 0], [0, 3], [0, 6]]
    out, mask, lengths, row_map = R.windows(*R.ragged([list(range(10, 21))]), 6, 1, **kw)
    assert out.tolist() == [[1, 10, 11, 12, 13, 2], [1, 13, 14, 15, 16, 2], [1, 16, 17, 18, 19, 2], [1, 19, 20, 2, 0, 0]]
    assert mask.tolist() == [[1] * 6] * 3 + [[1, 1, 1, 1, 0, 0]] and lengths.tolist() == [6, 6, 6, 4]
    assert row_map.tolist() == [[0, 0], [0, 3], [0, 6], [0, 9]]
    out, mask, lengths, row_map = R.windows(*R.ragged([[]]), 6, 1, **kw)
    assert out.tolist() == [[1, 2, 0, 0, 0, 0]] and mask.tolist() == [[1, 1, 0, 0, 0, 0]]
    assert lengths.tolist() == [2] and row_map.tolist() == [[0, 0]]
    out, mask, lengths, row_map = R.windows(*R.ragged([[7]]), 6, 1, padding_side="left", **kw)
    assert out.tolist() == [[0, 0, 0, 1, 7, 2]] and mask.tolist() == [[0, 0, 0, 1, 1, 1]]
    assert lengths.tolist() == [3] and row_map.tolist() == [[0, 0]]


def test_rows_follow_the_documents_and_row_offsets_is_their_prefix_sum():
    ids, offs = R.ragged([[5, 6, 7, 8, 9], [], [-1, -2], [1, 2, 3, 4]])
    out, mask, lengths, row_map = R.windows(ids, offs, 3, 1, eos_id=9, pad_id=-7, dtype=np.int64)  # C = 2, step = 1
    assert out.dtype == np.int64
    assert out.tolist() == [[5, 6, 9], [6, 7, 9], [7, 8, 9], [8, 9, 9], [9, -7, -7], [-1, -2, 9], [1, 2, 9], [2, 3, 9], [3, 4, 9]]
    assert lengths.tolist() == [3, 3, 3, 3, 1, 3, 3, 3, 3]
    assert row_map.tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [1, 0], [2, 0], [3, 0], [3, 1], [3, 2]]
    assert R.row_offsets(offs, 3, 1, eos_id=9).tolist() == [0, 4, 5, 6, 9]
    assert R.row_table(offs, 3, 1, eos_id=9)[0].tolist() == [0, 4, 5, 6, 9]
    empty = R.windows(*R.ragged([]), 4)
    assert [x.shape for x in empty] == [(0, 4), (0, 4), (0,), (0, 2)]
    assert [x.shape for x in R.windows_vec(*R.ragged([]), 4)] == [(0, 4), (0, 4), (0,), (0, 2)]


def test_vectorised_form_equals_the_loop_form():
    rnd = random.Random(5)
    for trial in range(150):
        docs = [[rnd.randrange(-3, 1000) for _ in range(rnd.choice((0, 1, 2, 3, 5, 8, 13, 40)))]
                for _ in range(rnd.randrange(0, 9))]
        ids, offs = R.ragged(docs)
        kw = rnd.choice(({}, {"eos_id": 99}, {"bos_id": -5}, {"bos_id": -5, "eos_id": 99}))
        L = rnd.randrange(len(kw) + 1, 12)
        stride = rnd.randrange(0, L - len(kw))
        for side in ("right", "left"):
            for dtype in (np.int32, np.int64):
                a = R.windows(ids, offs, L, stride, pad_id=-7, padding_side=side, dtype=dtype, **kw)
                b = R.windows_vec(ids, offs, L, stride, pad_id=-7, padding_side=side, dtype=dtype, **kw)
                assert all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b)), \
                    (trial, docs, L, stride, kw, side)
        assert np.array_equal(R.row_offsets(offs, L, stride, **kw), R.row_table(offs, L, stride, **kw)[0])


def test_rows_never_exceed_the_bound():
    rnd = random.Random(11)
    for s in (0, 1, 2):
        for L in range(s + 1, 12):
            for stride in range(0, L - s):
                lens = [rnd.randrange(0, 60) for _ in range(rnd.randrange(0, 7))] + [0, L - s, L - s + 1]
                offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                kw = {0: {}, 1: {"eos_id": 1}, 2: {"bos_id": 0, "eos_id": 1}}[s]
                n_rows = int(R.row_offsets(offs, L, stride, **kw)[-1])
                bound = _capi.windows_rows_bound(len(lens), int(offs[-1]), L, stride, s)
                assert bound == R.rows_bound(len(lens), int(offs[-1]), L, stride, s)
                assert len(lens) <= n_rows <= bound, (s, L, stride, lens)
                for n in range(0, 40):  # one document of every length
                    assert R.window_count(n, L - s, L - s - stride) <= _capi.windows_rows_bound(1, n, L, stride, s)


def test_reference_equals_tokenizers_overflowing_rows():
    tk = pytest.importorskip("tokenizers")
    from tokenizers import models, pre_tokenizers, processors
    words = ["w%d" % i for i in range(40)]
    vocab = {w: 10 + i for i, w in enumerate(words)}
    vocab.update({"[BOS]": 1, "[EOS]": 2, "[UNK]": 3})
    cases = 0
    for s in (0, 1, 2):
        tok = tk.Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
        tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
        kw = {}
        if s == 1:
            tok.post_processor = processors.TemplateProcessing(single="$A [EOS]", special_tokens=[("[EOS]", 2)])
            kw = {"eos_id": 2}
        elif s == 2:
            tok.post_processor = processors.TemplateProcessing(single="[BOS] $A [EOS]",
                                                               special_tokens=[("[BOS]", 1), ("[EOS]", 2)])
            kw = {"bos_id": 1, "eos_id": 2}
        for L in range(max(1, s + 1), 12):
            for stride in range(0, L - s):
                tok.enable_truncation(max_length=L, stride=stride)
                for n in range(0, 40):
                    enc = tok.encode(" ".join(words[:n]))
                    theirs = [enc.ids] + [o.ids for o in enc.overflowing]
                    out, _mask, lengths, _map = R.windows(*R.ragged([list(range(10, 10 + n))]), L, stride, pad_id=0, **kw)
                    ours = [row[:m].tolist() for row, m in zip(out, lengths)]
                    assert ours == theirs, (s, L, stride, n)
                    cases += 1
    assert cases == 6640


# ---- the Python surface: argument checks come before any device call ----------------------------------------------
def test_names_are_exported():
    for name in ("collate_windows", "batch_encode_windows"):
        assert name in hutoken_amd.__all__ and hasattr(hutoken_amd, name)
    for name in ("hutk_windows_rows_bound", "hutk_windows_rows_device", "hutk_collate_windows_device"):
        assert name in _capi.EXPORTS
        assert hasattr(_capi.load(), name)


def host_pair():
    import torch
    return torch.tensor([1, 2, 3], dtype=torch.int32), torch.tensor([0, 1, 3], dtype=torch.int64)


def test_collate_windows_argument_checks():
    import torch
    ids, offs = host_pair()
    with pytest.raises(ValueError, match="on the GPU"):  # host tensors: there is no CPU path
        hutoken_amd.collate_windows(ids, offs, 4)
    with pytest.raises(TypeError, match="torch tensor"):
        hutoken_amd.collate_windows([1, 2, 3], offs, 4)
    with pytest.raises(TypeError, match="torch tensor"):
        hutoken_amd.collate_windows(ids, np.array([0, 3]), 4)
    with pytest.raises(TypeError, match="int32"):
        hutoken_amd.collate_windows(ids.long(), offs, 4)
    with pytest.raises(TypeError, match="int64"):
        hutoken_amd.collate_windows(ids, offs.int(), 4)
    with pytest.raises(ValueError, match="one-dimensional"):
        hutoken_amd.collate_windows(ids.reshape(1, 3), offs, 4)
    for bad in (0, -1, 2**31):
        with pytest.raises(ValueError, match="max_length"):
            hutoken_amd.collate_windows(ids, offs, bad)
    with pytest.raises(ValueError, match="max_length"):  # max_length < s + 1: no room for a document id
        hutoken_amd.collate_windows(ids, offs, 2, bos_id=1, eos_id=2)
    with pytest.raises(ValueError, match="max_length"):
        hutoken_amd.collate_windows(ids, offs, 1, eos_id=2)
    for bad in (None, 2.0, "8", True):
        with pytest.raises(TypeError, match="max_length"):
            hutoken_amd.collate_windows(ids, offs, bad)
    with pytest.raises(TypeError):  # max_length is required
        hutoken_amd.collate_windows(ids, offs)
    for L, stride, kw in ((4, -1, {}), (4, 4, {}), (4, 5, {}), (4, 3, {"eos_id": 2}), (4, 2, {"bos_id": 1, "eos_id": 2}),
                          (1, 1, {})):
        with pytest.raises(ValueError, match="stride"):  # stride must stay below C = max_length - s
            hutoken_amd.collate_windows(ids, offs, L, stride, **kw)
    for bad in (None, 1.0, "1", True):
        with pytest.raises(TypeError, match="stride"):
            hutoken_amd.collate_windows(ids, offs, 4, bad)
    with pytest.raises(ValueError, match="padding_side"):
        hutoken_amd.collate_windows(ids, offs, 4, padding_side="both")
    with pytest.raises(TypeError):  # windows are cut on the right only: there is no truncation option
        hutoken_amd.collate_windows(ids, offs, 4, truncation="left")
    for bad in (torch.float32, torch.int16, "int8", np.int32):
        with pytest.raises(ValueError, match="dtype"):
            hutoken_amd.collate_windows(ids, offs, 4, dtype=bad)
    with pytest.raises(TypeError, match="bos_id"):
        hutoken_amd.collate_windows(ids, offs, 4, bos_id="1")
    with pytest.raises(TypeError, match="pad_id"):
        hutoken_amd.collate_windows(ids, offs, 4, pad_id=None)
    with pytest.raises(ValueError, match="eos_id"):
        hutoken_amd.collate_windows(ids, offs, 4, eos_id=2**31)
    with pytest.raises(ValueError, match="eos_id"):  # the C ABI's "absent" value
        hutoken_amd.collate_windows(ids, offs, 4, eos_id=-2**31)
    with pytest.raises(TypeError, match="n_rows"):
        hutoken_amd.collate_windows(ids, offs, 4, n_rows=2.0)
    with pytest.raises(ValueError, match="n_rows"):
        hutoken_amd.collate_windows(ids, offs, 4, n_rows=-1)
    with pytest.raises(TypeError):  # the options are keyword-only
        hutoken_amd.collate_windows(ids, offs, 4, 1, 1)


def rows_call(max_len, stride, bos=NO, eos=NO):
    return _capi.windows_rows_device(0, 0, 0, max_len, stride, bos, eos, 0)


def fill_call(max_len, stride, bos=NO, eos=NO, flags=0, out_width=4, n_docs=0, n_ids=0, n_rows=0):
    return _capi.collate_windows_device(0, 0, 0, n_docs, n_ids, n_rows, max_len, stride, bos, eos, 0, flags, out_width, 0)


def test_c_abi_argument_checks_need_no_device():
    # bad sizes are refused before the device is looked for
    for max_len, bos, eos in ((0, NO, NO), (-3, NO, NO), (1, NO, 2), (2, 1, 2), (2**31, 1, 2)):
        with pytest.raises(TypeError, match="max_len"):
            rows_call(max_len, 0, bos, eos)
        with pytest.raises(TypeError, match="max_len"):
            fill_call(max_len, 0, bos, eos)
        with pytest.raises(TypeError, match="max_len"):
            _capi.windows_rows_bound(1, 1, max_len, 0, (bos != NO) + (eos != NO))
    for max_len, stride, bos, eos in ((4, -1, NO, NO), (4, 4, NO, NO), (4, 3, NO, 2), (4, 2, 1, 2), (1, 1, NO, NO)):
        with pytest.raises(TypeError, match="stride"):
            rows_call(max_len, stride, bos, eos)
        with pytest.raises(TypeError, match="stride"):
            fill_call(max_len, stride, bos, eos)
        with pytest.raises(TypeError, match="stride"):
            _capi.windows_rows_bound(1, 1, max_len, stride, (bos != NO) + (eos != NO))
    assert _capi.load().hutk_windows_rows_bound(1, 1, 4, 4, 0) < 0  # the C function itself: a negative error
    assert _capi.load().hutk_windows_rows_bound(-1, 1, 4, 0, 0) < 0
    assert _capi.load().hutk_windows_rows_bound(1, 1, 4, 0, 3) < 0
    with pytest.raises(TypeError, match="bad arguments"):
        fill_call(4, 0, out_width=5)
    with pytest.raises(TypeError, match="bad arguments"):
        fill_call(4, 0, flags=4)  # an unknown bit
    with pytest.raises(TypeError, match="HUTK_COLLATE_PAD_LEFT"):
        fill_call(4, 0, flags=_capi.COLLATE_TRUNC_LEFT)  # windows are cut on the right only
    for kw in ({"n_docs": -1}, {"n_ids": -1}, {"n_rows": -1}):
        with pytest.raises(TypeError, match="bad arguments"):
            fill_call(4, 0, **kw)
    with pytest.raises(TypeError, match="bad arguments"):
        _capi.windows_rows_device(0, -1, 0, 4, 0, NO, NO, 0)
    assert _capi.windows_rows_bound(3, 10, 6, 1, 2) == 3 + 10 // 3
    assert _capi.windows_rows_bound(0, 0, 1, 0, 0) == 0


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        rows_call(4, 1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        fill_call(4, 1, flags=_capi.COLLATE_PAD_LEFT)


def test_text_entry_point_needs_an_initialised_context(monkeypatch):
    monkeypatch.setattr(hutoken_amd, "_ctx", None)
    with pytest.raises(RuntimeError, match="not initialized"):
        hutoken_amd.batch_encode_windows(["a"], 8, 2)
