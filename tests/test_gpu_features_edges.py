"""k_word_ids (csrc/hutk_features.hip) and k_rows_answers (csrc/hutk_collate.hip) on the geometry where they can go wrong:
document starts on tile, wavefront and thread edges, hundreds and thousands of starts in one tile, runs of empty
documents, word starts at chosen bits of the bitmap, spans of another split and of another text; rows of 1 to 4098
tokens, so that the wavefront search takes one, two and three rounds, with ties, overlaps and empty spans.

The inputs are laid out by tests/features_synth.py, which tests/test_features_synth_cpu.py holds to its claims; the
expected results are features_ref's.  Every comparison is exact and over every element; every call finds its output,
status and error word preset to -5.  Needs a real MI355X."""
import functools

import numpy as np
import pytest

import features_synth as FS
import spans_ref as S

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 4, 6
SENTINEL, GUARD = -5, 64
INT32_MAX = 2 ** 31 - 1
WIDTHS = ((4, np.int32), (8, np.int64))


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def cases():
    from hutoken_amd import _capi
    return FS.word_cases(_capi.word_ids_tile())


# ---- word ids ---------------------------------------------------------------------------------------------------------
def run_word_ids(b, width, dtype, spans=None, before=None):
    """hutk_token_word_ids_device on a WordBatch -> (words with a guard band either side, status, error word)"""
    import torch
    from hutoken_amd import _capi
    d_bits, d_before = dev(b.bits), dev(b.before) if before is None else before
    d_text, d_io = dev(b.text_offs), dev(b.id_offs)
    d_spans = dev((b.spans if spans is None else spans).astype(dtype).reshape(-1, 2))
    store = torch.full((GUARD + b.n_ids + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    words = store[GUARD:GUARD + b.n_ids]
    status = torch.full((b.n_docs + 1,), SENTINEL, dtype=torch.int32, device="cuda:0")
    err = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda:0")
    _capi.token_word_ids_device(d_bits.data_ptr(), d_before.data_ptr(), d_text.data_ptr(), b.n_docs, b.n_bytes, d_spans.data_ptr(), width,
                                d_io.data_ptr(), b.n_ids, words.data_ptr(), status.data_ptr(), err.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return store.cpu().numpy(), status.cpu().numpy(), int(err.item())


def check_word_ids(b, name, want_err=0, spans=None, want=None, before=None):
    want = b.words if want is None else want
    for width, dtype in WIDTHS:
        store, status, err = run_word_ids(b, width, dtype, spans, before)
        assert err == want_err, (name, width, err)
        assert (store[:GUARD] == SENTINEL).all() and (store[GUARD + b.n_ids:] == SENTINEL).all(), (name, width)
        got = store[GUARD:GUARD + b.n_ids]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, width, "%d ids differ, the first is id %d: %d, the restatement has %d"
                               % (bad.size, bad[0], got[bad[0]], want[bad[0]]))
        flags = [S.MISMATCH if d in b.flagged else 0 for d in range(b.n_docs)]
        assert status[:b.n_docs].tolist() == flags and status[b.n_docs] == SENTINEL, (name, width)


CASE_NAMES = ("edges, 0 empty", "edges, 1 empty", "edges, 3 empty", "3T one-token documents",
              "3T one-token documents, two empty behind each", "256 starts in tile 1", "257 starts in tile 1", "513 starts in tile 1",
              "runs of empties", "a long document", "no ids, 4 documents", "no documents", "sizes", "bit positions",
              "bit positions, lead 37, tail 50", "empty spans at a document's end")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_word_ids_geometry(name):
    from hutoken_amd import _capi
    T = _capi.word_ids_tile()
    names = ["%d ids" % n for n in (1, T - 1, T, T + 1)] if name == "sizes" else [name]
    for n in names:
        check_word_ids(cases()[n], n)


def test_every_case_is_run():
    from hutoken_amd import _capi
    T = _capi.word_ids_tile()
    assert set(cases()) == (set(CASE_NAMES) - {"sizes"}) | {"%d ids" % n for n in (1, T - 1, T, T + 1)}


def test_word_ids_with_the_prefix_counts_of_the_counting_call():
    """`before` from hutk_pretokenize_starts_device's counting call instead of numpy: the chain the Python function uses.
    First on a pre-tokeniser that has split nothing yet -- the bitmap is the caller's own, and the call once did nothing
    there --, then on the package's, whatever the tests before this one left in it, behind a split of sound offsets."""
    import importlib
    import torch
    import hutoken_amd as hutoken
    from hutoken_amd import _capi
    b = cases()["edges, 1 empty"]
    d_bits, d_text = dev(b.bits), dev(b.text_offs)
    stream = torch.cuda.current_stream().cuda_stream
    fresh = _capi.Pretokenizer(importlib.import_module("hutoken_amd.pretokenize").table_blob(), 0)
    try:
        before = torch.full((b.n_bytes // 32 + 2,), SENTINEL, dtype=torch.int64, device="cuda:0")
        fresh.starts_device(d_bits.data_ptr(), d_text.data_ptr(), b.n_docs, b.n_bytes, before.data_ptr(), 0, 0, stream)
        torch.cuda.synchronize()
        assert np.array_equal(before.cpu().numpy(), b.before)
        check_word_ids(b, "counted on the device", before=before)
    finally:
        fresh.close()
    text = dev(np.full(40, 97, dtype=np.uint8))
    hutoken.pretokenize_packed_device(text, dev(np.array([0, 40], dtype=np.int64)), "gpt2")
    before = torch.full((b.n_bytes // 32 + 2,), SENTINEL, dtype=torch.int64, device="cuda:0")
    hutoken._pretokenizer(d_bits.device).starts_device(d_bits.data_ptr(), d_text.data_ptr(), b.n_docs, b.n_bytes, before.data_ptr(), 0, 0, stream)
    torch.cuda.synchronize()
    assert np.array_equal(before.cpu().numpy(), b.before)
    check_word_ids(b, "counted on the device, the package's pre-tokeniser", before=before)


def test_word_starts_inside_tokens_are_reported_per_document():
    base = FS.mismatch_base()
    check_word_ids(base, "the batch as it is")
    for where, doc, token in FS.MISMATCHES:
        b, flagged = FS.with_inner_start(base, doc, token, where)
        assert flagged == [doc]
        check_word_ids(b, where, want_err=E_UNSUPPORTED)
    b, flagged = FS.with_inner_start(FS.with_inner_start(base, 1, 1, "a+1")[0], 3, 1, "b-1")
    assert flagged == [1, 3]
    check_word_ids(b, "two documents", want_err=E_UNSUPPORTED)
    for name, doc, pos in FS.CONTROLS:  # not strictly inside a non-empty span: nothing is flagged, the ids follow the new bit
        b = FS.with_start(base, doc, pos)
        assert not b.flagged
        check_word_ids(b, name)
    # across tiles: a flagged document in each of three tiles, the rest clean
    from hutoken_amd import _capi
    big = cases()["edges, 3 empty"]
    flagged = []
    for tile in range(3):  # the first token of two bytes or more from the tile's first id on
        k = next(k for k in range(tile * _capi.word_ids_tile(), big.n_ids) if big.spans[k, 1] - big.spans[k, 0] >= 2)
        d = int(np.searchsorted(big.id_offs, k, side="right")) - 1
        big, flagged = FS.with_inner_start(big, d, k - int(big.id_offs[d]), "a+1")
    assert len(flagged) == 3
    check_word_ids(big, "three tiles", want_err=E_UNSUPPORTED)


def test_spans_of_another_text_are_refused_and_nothing_else_is_touched():
    b = cases()["edges, 1 empty"]
    for name, k, spans in FS.foreign_spans(b):
        want = b.words.copy()
        want[k] = -1
        check_word_ids(b, name, want_err=E_ARG, spans=spans, want=want)


# ---- answer positions -------------------------------------------------------------------------------------------------
def run_answers(plan, side, spans, ans, width, dtype):
    """hutk_rows_answers_device -> (out [n_rows, 2] with a guard band either side, error word)"""
    import torch
    from hutoken_amd import _capi
    n = len(plan)
    d_plan, d_spans, d_ans = dev(plan), dev(spans.astype(dtype)), dev(ans.astype(dtype))
    store = torch.full((GUARD + 2 * n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda:0")
    out = store[GUARD:GUARD + 2 * n]
    err = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda:0")
    _capi.rows_answers_device(d_plan.data_ptr(), n, 1 if side == "b" else 0, d_spans.data_ptr(), width, len(spans), d_ans.data_ptr(),
                              len(ans), out.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = store.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + 2 * n:] == SENTINEL).all()
    return got[GUARD:GUARD + 2 * n].reshape(n, 2), int(err.item())


def check_answers(plan, side, spans, ans, what, want_err=0, want=None):
    want = FS.answers_fast(plan, side, spans, ans) if want is None else want
    for width, dtype in WIDTHS:
        got, err = run_answers(plan, side, spans, ans, width, dtype)
        assert err == want_err, (what, width, err)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (what, width, "%d rows differ, the first is row %d, answer %s: %s, the closed form has %s"
                               % (bad.size, bad[0], ans[plan[bad[0], 0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist()))
    return want


ANSWER_KS = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4098)


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("k", ANSWER_KS)
def test_answers_over_rows_of_k_tokens(k, side):
    plan, spans, ans = FS.answer_case(k, side)
    want = check_answers(plan, side, spans, ans, "k = %d" % k)
    found = int((want[:, 0] >= 0).sum())
    assert found * 10 >= len(plan) and (len(plan) - found) * 10 >= len(plan)


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 257])
def test_answers_row_counts(n_rows):
    plan, spans, ans = FS.answer_case(65, "b")
    found = FS.answers_fast(plan, "b", spans, ans)[:, 0] >= 0
    yes, no = np.nonzero(found)[0], np.nonzero(~found)[0]
    keep = np.where(np.arange(n_rows) % 2 == 0, np.resize(yes[::3], n_rows), np.resize(no[::3], n_rows))  # found and not found in turn
    want = check_answers(plan[keep], "b", spans, ans, "%d rows" % n_rows)
    assert (want[0::2, 0] >= 0).all() and (want[1::2, 0] < 0).all()


@pytest.mark.parametrize("k", [1, 65, 4097])
def test_answers_at_the_column_bound(k):
    """col = INT32_MAX - k is the last sound column: the answer columns are exact.  One more gives HUTK_E_ARG and (-1, -1)
    for that row alone."""
    for side in ("a", "b"):
        plan, spans, ans = FS.answer_case(k, side)
        c = 4 if side == "a" else 7
        found = np.nonzero(FS.answers_fast(plan, side, spans, ans)[:, 0] >= 0)[0]
        plan = plan[found[np.arange(6) * max(1, len(found) // 6) % len(found)]].copy()
        plan[1, c] = plan[4, c] = INT32_MAX - k
        want = check_answers(plan, side, spans, ans, "col = INT32_MAX - k")
        assert (want[[1, 4]] >= INT32_MAX - k).all() and want[:, 1].max() <= INT32_MAX - 1
        plan[2, c] = INT32_MAX - k + 1
        want[2] = -1
        check_answers(plan, side, spans, ans, "col = INT32_MAX - k + 1", want_err=E_ARG, want=want)


@pytest.mark.parametrize("k", [65, 4097])
def test_answers_through_the_python_function(k):
    import hutoken_amd
    for side, dtype in (("a", np.int64), ("b", np.int32)):
        plan, spans, ans = FS.answer_case(k, side)
        got = hutoken_amd.answer_positions(dev(plan), dev(spans.astype(dtype)), dev(ans.astype(dtype)), side=side, check=True)
        want = FS.answers_fast(plan, side, spans, ans)
        got = got.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
