"""Best-fit packing without a GPU: the restatement (tests/bestfit_ref.py) pinned to the worked example of
include/hutoken_amd.h by hand, its properties on random cases, the rows bound, the new names, and every refusal that
needs no device."""
import random

import numpy as np
import pytest

import bestfit_ref as R

A, B, C, D, E, F = range(6)
DOCS = [list(range(10, 15)), [], list(range(20, 29)), [30, 31, 32], [40], list(range(50, 57))]


def ragged(docs):
    ids = [x for d in docs for x in d]
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    return np.array(ids, dtype=np.int32), offs


def test_the_worked_example_by_hand():
    ids, offs = ragged(DOCS)
    got = R.pack(ids, offs, 8, eos_id=99, pad_id=0)
    assert got["input_ids"].tolist() == [[20, 21, 22, 23, 24, 25, 26, 27], [50, 51, 52, 53, 54, 55, 56, 99],
                                         [10, 11, 12, 13, 14, 99, 28, 99], [30, 31, 32, 99, 40, 99, 99, 0]]
    assert got["segment_ids"].tolist() == [[1] * 8, [1] * 8, [1, 1, 1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 2, 2, 3, 0]]
    assert got["position_ids"].tolist() == [list(range(8)), list(range(8)), [0, 1, 2, 3, 4, 5, 0, 1], [0, 1, 2, 3, 0, 1, 0, 0]]
    assert got["lengths"].tolist() == [8, 8, 8, 7]
    assert got["source"][2].tolist() == [0, 1, 2, 3, 4, -1, 13, -1]
    assert got["source"][3].tolist() == [14, 15, 16, -1, 17, -1, -1, -1]
    assert got["source"][0].tolist() == list(range(5, 13)) and got["source"][1].tolist() == list(range(18, 25)) + [-1]
    assert got["doc_map"].tolist() == [[-1, 0, 2, 0], [-1, 0, 3, 6], [0, 1, 2, 6], [-1, 0, 3, 0], [-1, 0, 3, 4], [1, 1, -1, -1]]
    assert got["info"] == (4, 2)
    assert got["input_ids"].dtype == np.int32 and got["source"].dtype == np.int64


def test_capacity_rows_are_padding():
    ids, offs = ragged(DOCS)
    got = R.pack(ids, offs, 8, eos_id=99, pad_id=7, rows_cap=6, dtype=np.int64)
    assert got["input_ids"].shape == (6, 8) and got["input_ids"].dtype == np.int64
    assert (got["input_ids"][4:] == 7).all() and (got["segment_ids"][4:] == 0).all() and got["lengths"][4:].tolist() == [0, 0]
    assert (got["source"][4:] == -1).all() and got["info"] == (4, 2)


def random_case(rng):
    L = rng.choice((1, 2, 3, 4, 7, 8, 64))
    bos, eos = rng.choice(((None, None), (None, 2), (1, 2)))
    s = (bos is not None) + (eos is not None)
    if L < max(1, s):
        L = 2
    kind = rng.randrange(3)
    n = rng.randrange(0, 50)
    lens = [rng.randrange(0, 3 * L + 7) if kind == 0 else rng.choice((0, 1, 2, L - 1, L, 2 * L, 3 * L + 5, L // 2))
            if kind == 1 else rng.randrange(0, L // 3 + 2) for _ in range(n)]
    docs = [[rng.randrange(10, 1000) for _ in range(k)] for k in lens]
    return L, bos, eos, s, docs


def test_properties_on_random_cases():
    """every non-empty sequence appears exactly once, contiguous and in order; only sequences longer than L are cut;
    segments count 1, 2, .. per row with 0 on padding only; lengths agree with the segments; the rows bound holds"""
    rng = random.Random(5)
    for _ in range(400):
        L, bos, eos, s, docs = random_case(rng)
        ids, offs = ragged(docs)
        got = R.pack(ids, offs, L, bos_id=bos, eos_id=eos, pad_id=0)
        n_rows, W = got["info"]
        assert got["input_ids"].shape == (n_rows, L)
        assert n_rows <= R.rows_bound(len(docs), len(ids), L, s), (L, s, [len(d) for d in docs])
        seg, pos, lens, src, dm = (got[k] for k in ("segment_ids", "position_ids", "lengths", "source", "doc_map"))
        covered = np.zeros((n_rows, L), dtype=np.int64)
        for i, d in enumerate(docs):
            seq = ([bos] if bos is not None else []) + d + ([eos] if eos is not None else [])
            first, n_whole, row, col = dm[i].tolist()
            assert n_whole == len(seq) // L and (first >= 0) == (n_whole > 0)
            assert (row >= 0) == (len(seq) % L > 0)
            if len(seq) <= L and seq:  # not cut: one piece
                assert (n_whole, len(seq)) == (1, L) or n_whole == 0
            parts = []
            if n_whole:
                assert first + n_whole <= W
                parts.append(got["input_ids"][first:first + n_whole].reshape(-1))
                covered[first:first + n_whole] += 1
                assert (seg[first:first + n_whole] == 1).all() and (pos[first:first + n_whole] == np.arange(L)).all()
            if row >= 0:
                n = len(seq) % L
                assert W <= row < n_rows and col + n <= L
                parts.append(got["input_ids"][row, col:col + n])
                covered[row, col:col + n] += 1
                assert pos[row, col:col + n].tolist() == list(range(n)) and len(set(seg[row, col:col + n].tolist())) == 1
                assert col == 0 or seg[row, col - 1] == seg[row, col] - 1
            assert np.concatenate(parts).tolist() == seq if parts else not seq
        assert (covered == (seg != 0)).all() and covered.max(initial=0) <= 1
        for r in range(n_rows):
            n = int(lens[r])
            assert (seg[r, :n] > 0).all() and (seg[r, n:] == 0).all() and (got["input_ids"][r, n:] == 0).all()
            assert seg[r, 0] == 1 and (np.diff(seg[r, :n]) >= 0).all() and (np.diff(seg[r, :n]) <= 1).all()
            assert n > 0 and (src[r, n:] == -1).all()
        real = src >= 0
        assert (got["input_ids"][real] == ids[src[real]]).all() and sorted(src[real].tolist()) == list(range(len(ids)))


def test_the_group_form_places_every_item_where_the_item_level_rule_does():
    """the walk over groups of identical bins -- the form the kernels use, here as tools/bench_bestfit.py's host plan --
    against the item-level restatement: random small cases, and log-normal lengths at L = 2048 and 8192"""
    import os
    import sys
    import helpers
    sys.path.insert(0, os.path.join(helpers.ROOT, "tools"))
    import bench_bestfit
    rng = random.Random(9)
    for _ in range(600):
        L, _bos, _eos, s, docs = random_case(rng)
        _ids, offs = ragged(docs)
        want = R.plan(offs, L, s)
        got, info = bench_bestfit.host_plan(offs, L, s)
        assert np.array_equal(got, want[0]) and info == (want[3] + len(want[2]), want[3]), (L, s, [len(d) for d in docs])
    lens = np.minimum(np.random.default_rng(0).lognormal(6.0, 1.2, 20000).astype(np.int64), 40000)
    offs = np.concatenate([[0], np.cumsum(lens)])
    for L in (2048, 8192):
        want = R.plan(offs, L, 1)
        got, info = bench_bestfit.host_plan(offs, L, 1)
        assert np.array_equal(got, want[0]) and info == (want[3] + len(want[2]), want[3])


def test_the_bound_is_tight_enough_and_never_low():
    """adversarial for the fill bound: items a little over half a row, which end alone in their bins"""
    for L in (2, 3, 8, 64):
        for n in (1, 2, 5, 33):
            docs = [[1] * (L // 2 + 1)] * n
            ids, offs = ragged(docs)
            got = R.pack(ids, offs, L)
            assert got["info"][0] <= R.rows_bound(n, len(ids), L, 0)
    assert R.rows_bound(0, 0, 8, 1) == 0


def test_library_bound_is_the_restated_one():
    from hutoken_amd import _capi
    rng = random.Random(2)
    for _ in range(200):
        n_docs, n_ids, L, s = rng.randrange(0, 10**6), rng.randrange(0, 10**9), rng.randrange(2, 65537), rng.randrange(3)
        assert _capi.bestfit_rows_bound(n_docs, n_ids, L, s) == R.rows_bound(n_docs, n_ids, L, s)
    assert _capi.bestfit_rows_bound(3, 2**40, 2048, 2) == R.rows_bound(3, 2**40, 2048, 2)
    for bad in ((-1, 0, 8, 0), (0, -1, 8, 0), (1, 1, 0, 0), (1, 1, 1, 2), (1, 1, 2**31, 0), (1, 1, 8, 3), (1, 1, 8, -1)):
        with pytest.raises(TypeError):
            _capi.bestfit_rows_bound(*bad)


def test_exports_and_all():
    import hutoken_amd as H
    from hutoken_amd import _capi
    for name in ("hutk_bestfit_rows_bound", "hutk_bestfit_plan_device", "hutk_bestfit_rows_device",
                 "hutk_rows_gather_source_device", "hutk_debug_bestfit_tile"):
        assert name in _capi.EXPORTS and name in _capi.SIGNATURES and hasattr(_capi.load(), name)
    for name in ("pack_best_fit", "gather_source", "batch_encode_best_fit"):
        assert name in H.__all__ and callable(getattr(H, name)) and name in H.__doc__
    assert _capi.bestfit_tile() == 256


def test_c_abi_refusals_need_no_device():
    """seq_len < 1, < s, >= 2^31 or above 65536, negative counts, a width other than 4 or 8, a per other than 1 or 2: HUTK_E_ARG
    (TypeError), before a device is looked for -- without a GPU a call that got further would raise RuntimeError"""
    from hutoken_amd import _capi
    NO = _capi.NO_TOKEN
    p = 4096  # (never dereferenced)
    for L, bos, eos in ((0, NO, NO), (-5, NO, NO), (1, 1, 2), (2**31, NO, NO), (65537, NO, NO)):
        with pytest.raises(TypeError, match="seq_len"):
            _capi.bestfit_plan_device(p, 1, 1, L, bos, eos, 4, p, p)
        with pytest.raises(TypeError, match="seq_len"):
            _capi.bestfit_rows_device(p, p, p, 1, 1, L, bos, eos, 0, 4, 4, p, p, p, p)
    for n_docs, n_ids, cap in ((-1, 0, 1), (0, -1, 1), (1, 1, -1), (2**31 - 1, 1, 1)):
        with pytest.raises(TypeError, match="negative"):
            _capi.bestfit_plan_device(p, n_docs, n_ids, 8, NO, NO, cap, p, p)
        with pytest.raises(TypeError, match="negative"):
            _capi.bestfit_rows_device(p, p, p, n_docs, n_ids, 8, NO, NO, 0, 4, cap, p, p, p, p)
    for width in (0, 2, 16):
        with pytest.raises(TypeError, match="out_width"):
            _capi.bestfit_rows_device(p, p, p, 1, 1, 8, NO, NO, 0, width, 4, p, p, p, p)
        with pytest.raises(TypeError, match="width is 4 or 8"):
            _capi.rows_gather_source_device(p, 1, p, 1, width, 1, 0, p)
    for per in (0, 3):
        with pytest.raises(TypeError, match="per is 1 or 2"):
            _capi.rows_gather_source_device(p, 1, p, 1, 4, per, 0, p)
    for n, n_values in ((-1, 1), (1, -1)):
        with pytest.raises(TypeError, match="negative"):
            _capi.rows_gather_source_device(p, n, p, n_values, 4, 1, 0, p)
    with pytest.raises(TypeError, match="fill"):
        _capi.rows_gather_source_device(p, 1, p, 1, 4, 1, 2**31, p)


def test_python_refusals_need_no_device():
    import torch
    import hutoken_amd as H
    ids, offs = torch.zeros(4, dtype=torch.int32), torch.tensor([0, 4])
    for kw, exc in ((dict(seq_len=0), ValueError), (dict(seq_len=1, bos_id=1, eos_id=2), ValueError), (dict(seq_len=2**31), ValueError),
                    (dict(seq_len=65537), ValueError), (dict(seq_len=8.0), TypeError), (dict(seq_len=True), TypeError),
                    (dict(seq_len=8, bos_id="a"), TypeError), (dict(seq_len=8, pad_id=None), TypeError),
                    (dict(seq_len=8, eos_id=2**31), ValueError), (dict(seq_len=8, dtype=torch.int16), ValueError),
                    (dict(seq_len=8, n_rows=-1), ValueError), (dict(seq_len=8, n_rows=1.5), TypeError)):
        with pytest.raises(exc):
            H.pack_best_fit(ids, offs, **kw)
    with pytest.raises(TypeError, match="torch tensor"):
        H.pack_best_fit([1, 2], offs, 8)
    with pytest.raises(TypeError, match="dtype"):
        H.pack_best_fit(ids.long(), offs, 8)
    with pytest.raises(ValueError, match="at least one entry"):
        H.pack_best_fit(ids, offs[:0], 8)
    with pytest.raises(ValueError, match="on the GPU"):
        H.pack_best_fit(ids, offs, 8)
    src, vals = torch.zeros((2, 3), dtype=torch.int64), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(TypeError, match="source"):
        H.gather_source([0], vals, 0)
    with pytest.raises(TypeError, match="int64"):
        H.gather_source(src.int(), vals, 0)
    with pytest.raises(ValueError, match="contiguous"):
        H.gather_source(src.t(), vals, 0)
    with pytest.raises(TypeError, match="values"):
        H.gather_source(src, vals.float(), 0)
    with pytest.raises(ValueError, match="values"):
        H.gather_source(src, torch.zeros((5, 3), dtype=torch.int32), 0)
    with pytest.raises(TypeError, match="fill"):
        H.gather_source(src, vals, 0.5)
    with pytest.raises(ValueError, match="fill"):
        H.gather_source(src, vals, 2**31)
    with pytest.raises(ValueError, match="on the GPU"):
        H.gather_source(src, vals, -100)
    with pytest.raises((ValueError, TypeError)):
        H.batch_encode_best_fit(["a"], 0)
    with pytest.raises(TypeError):
        H.batch_encode_best_fit(["a"], 8, eos_id="x")
