"""Collation without a GPU: the NumPy reference (tests/collate_ref.py) against expectations typed out by hand, its split
invariant, its vectorised forms against its loop forms, and the argument checks of the Python surface, which run before
any device call."""
import random

import numpy as np
import pytest

import collate_ref as R
import hutoken_amd
from hutoken_amd import _capi


def A(*rows):
    return np.array(rows, dtype=np.int32)


# ---- the reference itself, pinned by hand -----------------------------------------------------------------------
def test_padded_truncation_right_and_left_with_bos_and_eos():
    ids, offs = R.ragged([[10, 11, 12, 13, 14, 15]])
    out, mask, lengths = R.padded(ids, offs, 5, bos_id=1, eos_id=2, pad_id=0)
    assert out.tolist() == [[1, 10, 11, 12, 2]] and mask.tolist() == [[1, 1, 1, 1, 1]] and lengths.tolist() == [5]
    out, mask, lengths = R.padded(ids, offs, 5, bos_id=1, eos_id=2, pad_id=0, truncation="left")
    assert out.tolist() == [[1, 13, 14, 15, 2]] and mask.tolist() == [[1, 1, 1, 1, 1]] and lengths.tolist() == [5]


def test_padded_empty_documents_and_left_padding():
    ids, offs = R.ragged([[], [7]])
    out, mask, lengths = R.padded(ids, offs, 5, pad_id=9)  # s = 0: an empty document is all padding
    assert out.tolist() == [[9, 9, 9, 9, 9], [7, 9, 9, 9, 9]]
    assert mask.tolist() == [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0]] and lengths.tolist() == [0, 1]
    out, mask, lengths = R.padded(ids, offs, 5, bos_id=1, eos_id=2, pad_id=0)
    assert out.tolist() == [[1, 2, 0, 0, 0], [1, 7, 2, 0, 0]]
    assert mask.tolist() == [[1, 1, 0, 0, 0], [1, 1, 1, 0, 0]] and lengths.tolist() == [2, 3]
    out, mask, lengths = R.padded(ids, offs, 5, bos_id=1, eos_id=2, pad_id=0, padding_side="left")
    assert out.tolist() == [[0, 0, 0, 1, 2], [0, 0, 1, 7, 2]]
    assert mask.tolist() == [[0, 0, 0, 1, 1], [0, 0, 1, 1, 1]] and lengths.tolist() == [2, 3]
    out, mask, lengths = R.padded(*R.ragged([]), 3)
    assert out.shape == (0, 3) and mask.shape == (0, 3) and lengths.shape == (0,)
    out, _, _ = R.padded(ids, offs, 2, dtype=np.int64)
    assert out.dtype == np.int64


def test_packed_worked_example():
    p = R.Packer(4, eos_id=99, pad_id=0)
    rows = p.add(*R.ragged([[10, 11, 12], [], [20, 21, 22, 23, 24, 25], [30]]))
    assert np.array_equal(rows["input_ids"], A([10, 11, 12, 99], [99, 20, 21, 22], [23, 24, 25, 99]))
    assert np.array_equal(rows["position_ids"], A([0, 1, 2, 3], [0, 0, 1, 2], [0, 1, 2, 3]))
    assert np.array_equal(rows["segment_ids"], A([1, 1, 1, 1], [1, 2, 2, 2], [1, 1, 1, 1]))
    assert p.pending == 2
    tail = p.flush()
    assert np.array_equal(tail["input_ids"], A([30, 99, 0, 0]))
    assert np.array_equal(tail["position_ids"], A([0, 1, 0, 0]))
    assert np.array_equal(tail["segment_ids"], A([1, 1, 0, 0]))
    assert p.pending == 0 and p.flush()["input_ids"].shape == (0, 4)


def test_packed_a_sequence_across_two_row_boundaries():
    p = R.Packer(4, eos_id=99, pad_id=0)
    rows = p.add(*R.ragged([[10, 11, 12], [], [20, 21, 22, 23, 24, 25, 26, 27, 28, 29], [30]]))
    assert np.array_equal(rows["input_ids"], A([10, 11, 12, 99], [99, 20, 21, 22], [23, 24, 25, 26], [27, 28, 29, 99]))
    assert np.array_equal(rows["position_ids"], A([0, 1, 2, 3], [0, 0, 1, 2], [0, 1, 2, 3], [0, 1, 2, 3]))
    assert np.array_equal(rows["segment_ids"], A([1, 1, 1, 1], [1, 2, 2, 2], [1, 1, 1, 1], [1, 1, 1, 1]))
    tail = p.flush()
    assert np.array_equal(tail["input_ids"], A([30, 99, 0, 0]))
    assert np.array_equal(tail["position_ids"], A([0, 1, 0, 0]))
    assert np.array_equal(tail["segment_ids"], A([1, 1, 0, 0]))


def test_packed_without_tokens_adjacent_empty_documents_keep_segments_dense():
    p = R.Packer(4, pad_id=0)
    rows = p.add(*R.ragged([[1, 2], [], [], [3, 4, 5]]))
    assert np.array_equal(rows["input_ids"], A([1, 2, 3, 4]))
    assert np.array_equal(rows["position_ids"], A([0, 1, 0, 1]))
    assert np.array_equal(rows["segment_ids"], A([1, 1, 2, 2]))
    tail = p.flush()
    assert np.array_equal(tail["input_ids"], A([5, 0, 0, 0]))
    assert np.array_equal(tail["position_ids"], A([0, 0, 0, 0]))
    assert np.array_equal(tail["segment_ids"], A([1, 0, 0, 0]))


def random_docs(rng, n, longest=12, lo=-3, hi=50):
    return [[rng.randint(lo, hi) for _ in range(rng.choice([0, 0, 1, 2, 3, rng.randint(0, longest)]))] for _ in range(n)]


def pack_in_pieces(docs, cuts, L, **kw):
    p = R.Packer(L, **kw)
    parts = [p.add(*R.ragged(docs[a:b])) for a, b in zip([0] + cuts, cuts + [len(docs)])]
    parts.append(p.flush())
    return R.cat_rows(parts, L)


def test_packed_rows_do_not_depend_on_the_split():
    rng = random.Random(5)
    for trial in range(200):
        docs = random_docs(rng, rng.randint(0, 30))
        L = rng.choice([1, 2, 3, 4, 7, 16])
        kw = rng.choice([{}, {"eos_id": 99}, {"bos_id": 98, "eos_id": 99}, {"bos_id": 98}])
        cuts = sorted(rng.randint(0, len(docs)) for _ in range(rng.randint(0, 4)))  # 1 - 5 add calls
        assert R.rows_equal(pack_in_pieces(docs, [], L, **kw), pack_in_pieces(docs, cuts, L, **kw)), (trial, docs, L, kw, cuts)


def test_vectorised_forms_equal_the_loop_forms():
    rng = random.Random(6)
    for trial in range(150):
        docs = random_docs(rng, rng.randint(0, 40), longest=30)
        ids, offs = R.ragged(docs)
        kw = rng.choice([{}, {"eos_id": 99}, {"bos_id": 98, "eos_id": 99}, {"bos_id": 98}])
        dtype = rng.choice([np.int32, np.int64])
        L = rng.choice([1, 2, 3, 4, 7, 16, 64])
        p = R.Packer(L, pad_id=-7, dtype=dtype, **kw)
        whole, tail = p.add(ids, offs), p.flush()
        vw, vt = R.packed_vec(ids, offs, L, pad_id=-7, dtype=dtype, **kw)
        assert R.rows_equal(whole, vw) and R.rows_equal(tail, vt), (trial, docs, L, kw)
        L = max(L, len(kw))
        for tr in ("right", "left"):
            for side in ("right", "left"):
                a = R.padded(ids, offs, L, pad_id=-7, truncation=tr, padding_side=side, dtype=dtype, **kw)
                b = R.padded_vec(ids, offs, L, pad_id=-7, truncation=tr, padding_side=side, dtype=dtype, block=7, **kw)
                assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b)), (trial, docs, L, kw, tr, side)
        if len(docs) > 3:
            a = R.padded(ids, offs, L, **kw)
            b = R.padded_vec(ids, offs, L, rows=(1, len(docs) - 1), **kw)
            assert all(np.array_equal(x[1:-1], y) for x, y in zip(a, b))


# ---- the Python surface: argument checks come before any device call ----------------------------------------------
def test_names_are_exported():
    for name in ("collate_padded", "batch_encode_padded", "SequencePacker"):
        assert name in hutoken_amd.__all__ and hasattr(hutoken_amd, name)
    for name in ("hutk_collate_padded_device", "hutk_packer_create", "hutk_packer_rows", "hutk_packer_add_device",
                 "hutk_packer_flush_device", "hutk_packer_pending", "hutk_packer_destroy"):
        assert name in _capi.EXPORTS
        assert hasattr(_capi.load(), name)


def host_pair():
    import torch
    return torch.tensor([1, 2, 3], dtype=torch.int32), torch.tensor([0, 1, 3], dtype=torch.int64)


def test_collate_padded_argument_checks():
    import torch
    ids, offs = host_pair()
    with pytest.raises(ValueError, match="on the GPU"):  # host tensors: there is no CPU path
        hutoken_amd.collate_padded(ids, offs, 4)
    with pytest.raises(TypeError, match="torch tensor"):
        hutoken_amd.collate_padded([1, 2, 3], offs, 4)
    with pytest.raises(TypeError, match="torch tensor"):
        hutoken_amd.collate_padded(ids, np.array([0, 3]), 4)
    with pytest.raises(TypeError, match="int32"):
        hutoken_amd.collate_padded(ids.long(), offs, 4)
    with pytest.raises(TypeError, match="int64"):
        hutoken_amd.collate_padded(ids, offs.int(), 4)
    with pytest.raises(ValueError, match="one-dimensional"):
        hutoken_amd.collate_padded(ids.reshape(1, 3), offs, 4)
    for bad in (0, -1, 2**31):
        with pytest.raises(ValueError, match="max_length"):
            hutoken_amd.collate_padded(ids, offs, bad)
    with pytest.raises(ValueError, match="max_length"):  # bos and eos do not fit one element
        hutoken_amd.collate_padded(ids, offs, 1, bos_id=1, eos_id=2)
    for bad in (2.0, "8", True):
        with pytest.raises(TypeError, match="max_length"):
            hutoken_amd.collate_padded(ids, offs, bad)
    with pytest.raises(ValueError, match="truncation"):
        hutoken_amd.collate_padded(ids, offs, 4, truncation="middle")
    with pytest.raises(ValueError, match="padding_side"):
        hutoken_amd.collate_padded(ids, offs, 4, padding_side="both")
    for bad in (torch.float32, torch.int16, "int8", np.int32):
        with pytest.raises(ValueError, match="dtype"):
            hutoken_amd.collate_padded(ids, offs, 4, dtype=bad)
    with pytest.raises(TypeError, match="bos_id"):
        hutoken_amd.collate_padded(ids, offs, 4, bos_id="1")
    with pytest.raises(TypeError, match="pad_id"):
        hutoken_amd.collate_padded(ids, offs, 4, pad_id=None)
    with pytest.raises(ValueError, match="eos_id"):
        hutoken_amd.collate_padded(ids, offs, 4, eos_id=2**31)
    with pytest.raises(ValueError, match="eos_id"):  # the C ABI's "absent" value
        hutoken_amd.collate_padded(ids, offs, 4, eos_id=-2**31)
    with pytest.raises(TypeError):  # the options are keyword-only
        hutoken_amd.collate_padded(ids, offs, 4, 1)


def test_sequence_packer_argument_checks():
    import torch
    for bad in (0, -5, 2**31):
        with pytest.raises(ValueError, match="seq_len"):
            hutoken_amd.SequencePacker(bad)
    for bad in (None, 4.0, "4", True):
        with pytest.raises(TypeError, match="seq_len"):
            hutoken_amd.SequencePacker(bad)
    with pytest.raises(ValueError, match="dtype"):
        hutoken_amd.SequencePacker(8, dtype=torch.float16)
    with pytest.raises(TypeError, match="eos_id"):
        hutoken_amd.SequencePacker(8, eos_id=1.5)
    with pytest.raises(ValueError, match="pad_id"):
        hutoken_amd.SequencePacker(8, pad_id=2**40)
    with pytest.raises(TypeError):
        hutoken_amd.SequencePacker(8, 50256)  # keyword-only


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        hutoken_amd.SequencePacker(8, eos_id=1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.collate_padded_device(0, 0, 0, 0, 4, _capi.NO_TOKEN, _capi.NO_TOKEN, 0, 0, 4, 0)


def test_text_entry_points_need_an_initialised_context(monkeypatch):
    monkeypatch.setattr(hutoken_amd, "_ctx", None)
    with pytest.raises(RuntimeError, match="not initialized"):
        hutoken_amd.batch_encode_padded(["a"], 8)
    with pytest.raises(RuntimeError, match="not initialized"):
        hutoken_amd.SequencePacker.add_texts(object.__new__(hutoken_amd.SequencePacker), ["a"])


def test_c_abi_argument_checks_need_no_device():
    # bad sizes are refused before the device is looked for
    for max_len, bos, eos in ((0, _capi.NO_TOKEN, _capi.NO_TOKEN), (1, 1, 2), (2**31, 1, 2)):
        with pytest.raises(TypeError, match="max_len"):
            _capi.collate_padded_device(0, 0, 0, 0, max_len, bos, eos, 0, 0, 4, 0)
    with pytest.raises(TypeError, match="bad arguments"):
        _capi.collate_padded_device(0, 0, 0, 0, 4, 1, 2, 0, 0, 5, 0)  # out_width
    with pytest.raises(TypeError, match="seq_len"):
        _capi.Packer(0)
    with pytest.raises(TypeError, match="seq_len"):
        _capi.Packer(8, out_width=2)
