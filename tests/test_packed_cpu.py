"""Packed rows for training without a GPU: the restatement (packed_ref) on the worked example of include/hutoken_amd.h
and DESIGN.md section 8j, its invariance over add splits, the exports, and every refusal that needs no device."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import collate_ref as CR
import packed_ref as R
import hutoken_amd as H
from hutoken_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGN = -100
NEW_SYMBOLS = ("hutk_packer_create_channels", "hutk_packer_channel_count", "hutk_packer_add_channels_device",
               "hutk_packer_flush_channels_device", "hutk_packed_cu_seqlens_device", "hutk_packed_labels_device",
               "hutk_debug_cu_tile")


# ---- the worked example ------------------------------------------------------------------------------------------------
def worked():
    ids, offsets = CR.ragged([[10, 11, 12], [], [20, 21, 22, 23, 24, 25], [30]])
    p = R.Packer(4, eos_id=99, pad_id=0, channels=[(np.int64, 1, IGN)])
    return p.add(ids, offsets, [ids.astype(np.int64)]), p.flush()


def test_worked_example_rows_by_hand():
    done, rest = worked()
    assert done["input_ids"].tolist() == [[10, 11, 12, 99], [99, 20, 21, 22], [23, 24, 25, 99]]
    assert done["segment_ids"].tolist() == [[1, 1, 1, 1], [1, 2, 2, 2], [1, 1, 1, 1]]
    assert done["channels"][0].tolist() == [[10, 11, 12, IGN], [IGN, 20, 21, 22], [23, 24, 25, IGN]]
    assert done["channels"][0].dtype == np.int64
    assert rest["input_ids"].tolist() == [[30, 99, 0, 0]]
    assert rest["segment_ids"].tolist() == [[1, 1, 0, 0]]
    assert rest["channels"][0].tolist() == [[30, IGN, IGN, IGN]]


def test_worked_example_cu_seqlens_and_labels_by_hand():
    done, rest = worked()
    rows = R.cat([done, rest])
    cu, info = R.cu_seqlens(rows["segment_ids"], 8)
    assert cu.tolist() == [0, 4, 5, 8, 12, 14, 16, 16, 16] and info == (6, 4) and cu.dtype == np.int32
    assert R.cu_seqlens_vec(rows["segment_ids"], 8)[0].tolist() == cu.tolist()
    i = IGN
    want = [[11, 12, 99, i], [i, 21, 22, i], [24, 25, 99, i], [99, i, i, i]]
    assert R.labels(rows["input_ids"], rows["segment_ids"], True, i).tolist() == want
    assert R.labels_vec(rows["input_ids"], rows["segment_ids"], True, i).tolist() == want
    assert R.labels(rows["input_ids"], rows["segment_ids"], False, -1).tolist() == \
        [[10, 11, 12, 99], [99, 20, 21, 22], [23, 24, 25, 99], [30, 99, -1, -1]]
    # a capacity below the count: the first starts, the total behind them, the true count
    cu, info = R.cu_seqlens(rows["segment_ids"], 3)
    assert cu.tolist() == [0, 4, 5, 16] and info == (6, 11)
    assert R.cu_seqlens(np.zeros((0, 4), np.int32), 2)[0].tolist() == [0, 0, 0]
    assert R.cu_seqlens(np.zeros((0, 4), np.int32), 2)[1] == (0, 0)


def test_worked_example_is_in_the_header_and_the_design():
    for path in (("include", "hutoken_amd.h"), ("DESIGN.md",)):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, *path)).read().replace("*", " "))
        for needle in ("30 -100 -100 -100", "0 4 5 8 12 14 16 16 16", "99 i i i"):
            assert needle in text, (path, needle)


# ---- the restatement against itself --------------------------------------------------------------------------------------
def random_case(rng, n_docs, bos, eos):
    docs = [[rng.randrange(10, 1000) for _ in range(rng.choice((0, 0, 1, 2, 3, 5, 9, 17)))] for _ in range(n_docs)]
    ids, offsets = CR.ragged(docs)
    n = len(ids)
    values = [np.arange(n, dtype=np.int32) * 3 + 1, -np.arange(n, dtype=np.int64) - 2**33,
              np.stack([np.arange(n), np.arange(n) + 7], axis=1).astype(np.int32),
              np.stack([np.arange(n) * 2**32, -np.arange(n)], axis=1).astype(np.int64)]
    channels = [(np.int32, 1, -1), (np.int64, 1, IGN), (np.int32, 2, 0), (np.int64, 2, -2**40)]
    return ids, offsets, values, channels


@pytest.mark.parametrize("bos,eos", [(None, None), (None, 2), (1, 2)])
def test_rows_do_not_depend_on_the_add_splits(bos, eos):
    rng = random.Random(5)
    for L in (1, 3, 4, 7):
        ids, offsets, values, channels = random_case(rng, 40, bos, eos)
        whole = R.Packer(L, bos, eos, 9, channels=channels)
        one = R.cat([whole.add(ids, offsets, values), whole.flush()])
        # the id rows are the parent's
        base = CR.Packer(L, bos, eos, 9)
        assert CR.rows_equal(CR.cat_rows([base.add(ids, offsets), base.flush()], L), one)
        for cuts in ([20], [1, 2, 3, 39], list(range(1, 40))):
            p = R.Packer(L, bos, eos, 9, channels=channels)
            parts = []
            for a, b in zip([0] + cuts, cuts + [40]):
                o = offsets[a:b + 1]
                parts.append(p.add(ids[o[0]:o[-1]], o - o[0], [v[o[0]:o[-1]] for v in values]))
            parts.append(p.flush())
            got = R.cat(parts)
            assert CR.rows_equal(got, one)
            for x, y in zip(got["channels"], one["channels"]):
                assert x.dtype == y.dtype and np.array_equal(x, y)
        # a channel equal to the ids is the id rows, with the fill where the packer put a token of its own
        p = R.Packer(L, bos, eos, 9, channels=[(np.int32, 1, -5)])
        rows = R.cat([p.add(ids, offsets, [ids]), p.flush()])
        own = np.isin(rows["input_ids"], [x for x in (bos, eos) if x is not None]) | (rows["segment_ids"] == 0)
        assert np.array_equal(rows["channels"][0], np.where(own, -5, rows["input_ids"]))


def test_loop_and_vectorised_forms_agree():
    rng = np.random.default_rng(3)
    for n_rows, L in ((1, 1), (5, 1), (3, 7), (6, 16)):
        seg = rng.integers(0, 3, size=(n_rows, L)).astype(np.int32)
        values = rng.integers(-50, 50, size=(n_rows, L)).astype(np.int64)
        for cap in (0, 1, n_rows, n_rows * L, n_rows * L + 3):
            a, b = R.cu_seqlens(seg, cap), R.cu_seqlens_vec(seg, cap)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        for shift in (False, True):
            assert np.array_equal(R.labels(values, seg, shift, -7), R.labels_vec(values, seg, shift, -7))


# ---- exports ---------------------------------------------------------------------------------------------------------
def test_names_are_exported():
    for name in ("packed_cu_seqlens", "packed_lm_labels", "SequencePacker"):
        assert name in H.__all__ and hasattr(H, name)
    header = open(os.path.join(ROOT, "include", "hutoken_amd.h")).read()
    lib = _capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _capi.EXPORTS and hasattr(lib, name)
    assert "#define HUTK_PACKER_MAX_CHANNELS 4" in header and _capi.PACKER_MAX_CHANNELS == 4
    assert _capi.cu_tile() >= 256 and _capi.cu_tile() % 256 == 0


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def test_channel_specs_are_checked_before_any_device_call():
    import torch
    P = H.SequencePacker
    with pytest.raises(TypeError, match="channels must be a dict"):
        P(8, channels=[("labels", "int64", -100)])
    with pytest.raises(TypeError, match=r"\(dtype, fill\)"):
        P(8, channels={"labels": "int64"})
    with pytest.raises(TypeError, match=r"\(dtype, fill\)"):
        P(8, channels={"labels": ("int64", 0, 1, 2)})
    with pytest.raises(ValueError, match="dtype must be torch.int32 or torch.int64"):
        P(8, channels={"labels": (torch.float32, 0)})
    with pytest.raises(ValueError, match="dtype must be torch.int32 or torch.int64"):
        P(8, channels={"labels": ("uint8", 0)})
    with pytest.raises(TypeError, match="fill must be an int"):
        P(8, channels={"labels": ("int64", 0.5)})
    with pytest.raises(TypeError, match="fill must be an int"):
        P(8, channels={"labels": ("int64", True)})
    with pytest.raises(ValueError, match="fill must fit int32"):
        P(8, channels={"labels": (torch.int32, 2**31)})
    with pytest.raises(ValueError, match="fill must fit int64"):
        P(8, channels={"labels": ("int64", -2**63 - 1)})
    with pytest.raises(ValueError, match="per .* must be 1 or 2"):
        P(8, channels={"spans": ("int32", 0, 3)})
    with pytest.raises(TypeError, match="name must be a non-empty str"):
        P(8, channels={3: ("int32", 0)})
    for name in ("input_ids", "position_ids", "segment_ids"):
        with pytest.raises(ValueError, match="cannot be named"):
            P(8, channels={name: ("int32", 0)})
    with pytest.raises(ValueError, match="at most 4 channels"):
        P(8, channels={"c%d" % i: ("int32", 0) for i in range(5)})
    # what is accepted: both spellings of a dtype, per given or not
    specs = H._channel_specs({"labels": ("int64", -100), "spans": (torch.int32, 0, 2)})
    assert specs == [("labels", "int64", 8, 1, -100), ("spans", "int32", 4, 2, 0)]
    assert H._channel_specs(None) == [] and H._channel_specs({}) == []


def packer_with(channels):
    p = H.SequencePacker.__new__(H.SequencePacker)  # (no device: only the checks in front of it are run)
    p.seq_len, p._channels = 8, H._channel_specs(channels)
    return p


def test_channel_tensors_are_checked_before_any_device_call():
    import torch
    p = packer_with({"labels": ("int64", -100), "spans": ("int32", 0, 2)})
    ids, offsets = torch.zeros(6, dtype=torch.int32), torch.tensor([0, 6])
    lab, spans = torch.zeros(6, dtype=torch.int64), torch.zeros((6, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match=r"missing \['labels', 'spans'\]"):
        p.add(ids, offsets)
    with pytest.raises(ValueError, match=r"missing \['spans'\]"):
        p.add(ids, offsets, channels={"labels": lab})
    with pytest.raises(ValueError, match=r"not declared \['words'\]"):
        p.add(ids, offsets, channels={"labels": lab, "spans": spans, "words": lab})
    with pytest.raises(TypeError, match="channels must be a dict"):
        p.add(ids, offsets, channels=[lab, spans])
    with pytest.raises(TypeError, match="'labels' must be a torch tensor"):
        p.add(ids, offsets, channels={"labels": [0] * 6, "spans": spans})
    with pytest.raises(TypeError, match="'labels' must have dtype int64"):
        p.add(ids, offsets, channels={"labels": lab.to(torch.int32), "spans": spans})
    with pytest.raises(TypeError, match="'spans' must have dtype int32"):
        p.add(ids, offsets, channels={"labels": lab, "spans": spans.to(torch.int64)})
    with pytest.raises(ValueError, match=r"'spans' must be contiguous and of shape \[m, 2\]"):
        p.add(ids, offsets, channels={"labels": lab, "spans": spans[:, 0].contiguous()})
    with pytest.raises(ValueError, match=r"'labels' must be contiguous and of shape \[m\]"):
        p.add(ids, offsets, channels={"labels": torch.zeros((6, 2), dtype=torch.int64), "spans": spans})
    with pytest.raises(ValueError, match=r"'labels' must be contiguous"):
        p.add(ids, offsets, channels={"labels": torch.zeros(12, dtype=torch.int64)[::2], "spans": spans})
    with pytest.raises(ValueError, match="fewer than n_ids = 6"):
        p.add(ids, offsets, n_ids=6, channels={"labels": lab[:5], "spans": spans})
    # all of that passes: the next thing wrong is that nothing is on a GPU
    with pytest.raises(ValueError, match="must be on the GPU"):
        p.add(ids, offsets, n_ids=6, channels={"labels": lab, "spans": spans})
    # a packer without channels takes none
    with pytest.raises(ValueError, match=r"not declared \['labels'\]"):
        packer_with(None).add(ids, offsets, channels={"labels": lab})


def test_add_texts_refuses_a_packer_with_channels():
    with pytest.raises(ValueError, match="texts carry none"):
        packer_with({"labels": ("int64", -100)}).add_texts(["a"])


def create(n, widths, per, fills, seq_len=8):
    h = C.c_void_p()
    arr = lambda t, v: (t * max(1, len(v)))(*v)  # noqa: E731
    return _capi.load().hutk_packer_create_channels(C.byref(h), seq_len, _capi.NO_TOKEN, _capi.NO_TOKEN, 0, 4, -1, n,
                                                    arr(C.c_int, widths), arr(C.c_int, per), arr(C.c_int64, fills))


def test_create_channels_refuses_bad_specs_before_any_device_call():
    for n, widths, per, fills in ((5, [4] * 5, [1] * 5, [0] * 5), (-1, [4], [1], [0]), (1, [2], [1], [0]), (1, [16], [1], [0]),
                                  (2, [4, 8], [1, 3], [0, 0]), (1, [4], [0], [0]), (1, [4], [1], [2**31]),
                                  (2, [8, 4], [1, 2], [2**40, -2**31 - 1])):
        assert create(n, widths, per, fills) == _capi.E_ARG, (n, widths, per, fills)
        assert "hutk_packer_create_channels" in _capi.last_error()
    h = C.c_void_p()
    lib = _capi.load()
    assert lib.hutk_packer_create_channels(C.byref(h), 8, _capi.NO_TOKEN, _capi.NO_TOKEN, 0, 4, -1, 1, None, None, None) == _capi.E_ARG
    assert create(1, [4], [1], [0], seq_len=0) == _capi.E_ARG
    assert lib.hutk_packer_channel_count(None) == -1


def test_cu_seqlens_refuses_what_does_not_fit_int32():
    import torch
    lib = _capi.load()
    for n_rows, L in ((2**31, 1), (1, 2**31), (2**16, 2**15), (2**20, 2**20), (-1, 4), (4, 0)):
        assert lib.hutk_packed_cu_seqlens_device(None, n_rows, L, 4, None, None, None, None) == _capi.E_ARG, (n_rows, L)
        assert "hutk_packed_cu_seqlens_device" in _capi.last_error()
    with pytest.raises(TypeError, match="dtype int32"):
        H.packed_cu_seqlens(torch.zeros((2, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"\[n_rows, L\]"):
        H.packed_cu_seqlens(torch.zeros(8, dtype=torch.int32))
    with pytest.raises(TypeError, match="cap must be an int"):
        H.packed_cu_seqlens(torch.zeros((2, 4), dtype=torch.int32), cap=2.0)
    with pytest.raises(ValueError, match="cap must be in"):
        H.packed_cu_seqlens(torch.zeros((2, 4), dtype=torch.int32), cap=-1)
    with pytest.raises(ValueError, match="must be on the GPU"):
        H.packed_cu_seqlens(torch.zeros((2, 4), dtype=torch.int32), cap=8)


def test_packed_lm_labels_argument_checks():
    import torch
    seg = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(TypeError, match="values must have dtype int32 or int64"):
        H.packed_lm_labels(seg.to(torch.int16), seg)
    with pytest.raises(TypeError, match="segment_ids must have dtype int32"):
        H.packed_lm_labels(seg, seg.to(torch.int64))
    with pytest.raises(ValueError, match="shape of values"):
        H.packed_lm_labels(seg, seg[:1])
    with pytest.raises(TypeError, match="shift must be a bool"):
        H.packed_lm_labels(seg, seg, shift=1)
    with pytest.raises(ValueError, match="ignore_index must fit int32"):
        H.packed_lm_labels(seg, seg, ignore_index=2**31)
    with pytest.raises(ValueError, match="must be on the GPU"):
        H.packed_lm_labels(seg, seg, shift=True)
    lib = _capi.load()
    assert lib.hutk_packed_labels_device(None, 2, None, 1, 4, 0, 0, None, None) == _capi.E_ARG      # the width
    assert lib.hutk_packed_labels_device(None, 4, None, 1, 4, 0, 2**31, None, None) == _capi.E_ARG  # ignore_index
    assert lib.hutk_packed_labels_device(None, 4, None, 1, 4, 0, 0, None, None) == _capi.E_ARG      # NULL buffers
