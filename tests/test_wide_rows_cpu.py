"""tests/wide_rows.py held to its claims without a GPU, at the boundaries 2^16 and 2^17: the band straddles the boundary,
the sync points of the packed stream are where they are said to be, the chat and fill-in-the-middle blocks lay the named
structures across p, the torch references equal the numpy ones, a batch of copies gives copies of the block's result --
and every checker FAILS, naming the position, when one element past the boundary of a correct result is changed, every
invariant when the rows past the boundary are a copy of row 0 (a wrapped index) or the last row is left at the guard
value.  This file is the evidence that tests/test_gpu_wide_rows.py would notice a wrong kernel."""
import itertools
import re

import numpy as np
import pytest
import torch

import chat_ref
import collate_ref
import features_ref
import fim_ref
import packed_ref
import span_ref
import targets_ref as T
import wide_cases as W
import wide_rows as WR

BOUNDARIES = (2 ** 16, 2 ** 17)
LENGTHS = (64, 61)  # the boundary falls on a row's first element, and inside a row
SEED = 21


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


class Rows:
    """the padded batch of wide_rows.padded_docs by the numpy references"""

    def __init__(self, B, L):
        self.B, self.L = B, L
        self.lens, self.offs, self.truncated, self.empty = WR.padded_docs(B, L)
        self.n = len(self.lens)
        self.ids = WR.draw_ids(int(self.offs[-1])).numpy()
        tpl = dict(bos_id=WR.BOS, eos_id=WR.EOS, truncation="left")
        self.rows, self.mask, self.lengths = collate_ref.padded_vec(self.ids, self.offs, L, pad_id=WR.PAD, **tpl)
        self.plan = features_ref.padded_plan(self.offs, L, **tpl)
        self.k = B // L  # the row that holds flat element B


_rows = {}


def rows_of(B, L):
    if (B, L) not in _rows:
        _rows[B, L] = Rows(B, L)
    return _rows[B, L]


CASES = [pytest.param(B, L, id="%d-%d" % (B, L)) for B in BOUNDARIES for L in LENGTHS]


def fails_at(fn, flat, B):
    """fn raises an AssertionError that names flat position `flat` and the far side of the boundary"""
    with pytest.raises(AssertionError) as e:
        fn()
    text = str(e.value)
    assert re.search(r"flat position %d\b" % flat, text) and "at or past %d" % B in text, text


def wrapped(x, k):
    """the rows from k on replaced by a copy of row 0"""
    y = x.clone()
    y[k:] = x[0]
    return y


def unwritten(x):
    """the last row left at the guard value"""
    y = x.clone()
    y[-1] = WR.GUARD_VALUE
    return y


# ---- the shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", CASES)
def test_the_band_straddles_the_boundary(B, L):
    r = rows_of(B, L)
    a, b = WR.band(B, L)
    assert r.n == WR.rows_shape(B, L) == b and r.n * L > B
    assert a * L < B - 32 * L and (r.k + 1) * L > B >= r.k * L and (r.n - 63) * L > B and r.n - 64 == r.k
    assert (B % L != 0) == (L == 61)
    for rows, length in ((r.truncated, L), (r.empty, 2)):
        assert any(x < r.k for x in rows) and any(x > r.k for x in rows) and all(a <= x < b for x in rows)
        assert all(r.lengths[x] == length for x in rows)
    assert len(set(r.lengths[[0, r.k, r.n - 1]].tolist())) == 3
    assert (r.lens == 5000).sum() >= 40 and r.ids.min() >= WR.ID_LO and r.ids.max() < WR.ID_HI
    assert WR.side(B - 1, B) == "below %d" % B and WR.side(B, B) == "at or past %d" % B
    assert "negative as int32" in WR.side(W.B31, W.B31) and "wraps" in WR.side(W.B32 + 5, W.B32) and WR.side(5, W.B32) == "below 2^32"


# ---- the deterministic passes: torch against numpy, and the checker ---------------------------------------------------
FLAG_SETS = [sum(c) for n in range(1, 5) for c in itertools.combinations((1, 2, 4, 8), n)]


@pytest.mark.parametrize("B,L", CASES)
def test_torch_lm_labels_equals_labels_ref(B, L):
    r = rows_of(B, L)
    for flags in FLAG_SETS:
        for shift in (0, T.LABELS_SHIFT):
            want, wrong = T.labels_ref(r.rows, r.mask, r.plan, flags | shift, WR.IGN)
            assert not wrong
            got = WR.torch_lm_labels(t(r.rows), t(r.mask), t(r.plan), flags | shift)
            assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want), (flags, shift)
    # a plan of two sides (pairs): the B side, the separators between and the eos behind it
    plan = r.plan[:50].copy()
    plan[:, 3] = np.minimum(plan[:, 3], 5)
    plan[:, 6], plan[:, 7] = 4, plan[:, 4] + plan[:, 3] + 2
    mask = (np.arange(L)[None, :] < (plan[:, 7] + 5)[:, None]).astype(np.uint8)
    for flags in FLAG_SETS:
        want, wrong = T.labels_ref(r.rows[:50], mask, plan, flags | T.LABELS_SHIFT, WR.IGN)
        assert not wrong
        assert np.array_equal(WR.torch_lm_labels(t(r.rows[:50]), t(mask), t(plan), flags | T.LABELS_SHIFT).numpy(), want)


@pytest.mark.parametrize("B,L", CASES)
def test_torch_gather_equals_features_ref_and_the_checker_names_the_element(B, L):
    r = rows_of(B, L)
    v4, v16 = WR.gather_values(len(r.ids))
    for values, fill in ((v4, WR.FILL4), (v16, WR.FILL16)):
        want = features_ref.gather(r.plan, L, values.numpy(), fill=fill)
        got = WR.torch_gather(t(r.plan), L, values, fill)
        assert got.dtype == values.dtype and np.array_equal(got.numpy(), want)
        ref = lambda a, b: WR.torch_gather(t(r.plan[a:b]), L, values, fill)  # noqa: E731
        WR.assert_rect(got, ref, B, "gather", slice_rows=100)
        per = got[0].numel()
        bad = got.clone()
        bad.view(-1)[(r.k + 1) * per + 3] += 1  # (a token's column: column 0 holds bos)
        fails_at(lambda: WR.assert_rect(bad, ref, B, "gather", slice_rows=100), (r.k + 1) * per + 3, B)
        fails_at(lambda: WR.assert_band(bad, want[r.k - 5:], r.k - 5, B, "gather"), (r.k + 1) * per + 3, B)
        WR.assert_band(got, want[r.k - 5:], r.k - 5, B, "gather")
        for broken in (wrapped(got, r.k), unwritten(got)):
            with pytest.raises(AssertionError):
                WR.assert_rect(broken, ref, B, "gather", slice_rows=100)


@pytest.mark.parametrize("L", LENGTHS + (7,))
def test_torch_packed_labels_equals_packed_ref(L):
    seg = WR.segment_rows(1000, 1060, L)
    assert seg.dtype == torch.int32 and (seg == 0).any() and int(seg.max()) >= min(4, L // 5) and (seg[:, 0] == 1).all()
    assert np.array_equal(WR.segment_rows(1010, 1020, L).numpy(), seg[10:20].numpy())  # (a function of the row's number)
    values = torch.randint(-5, 50000, seg.shape, dtype=torch.int32, generator=torch.Generator().manual_seed(1))
    for shift in (False, True):
        want = packed_ref.labels(values.numpy(), seg.numpy(), shift, WR.IGN)
        assert np.array_equal(WR.torch_packed_labels(values, seg, shift).numpy(), want)


# ---- the random passes ------------------------------------------------------------------------------------------------
def words_of(r):
    w = np.arange(len(r.ids), dtype=np.int64) // 3
    w[::11] = -1  # protected
    return w.astype(np.int32)


@pytest.mark.parametrize("whole_word", [False, True], ids=["tokens", "words"])
@pytest.mark.parametrize("B,L", CASES)
def test_mlm_band_and_invariants(B, L, whole_word):
    r = rows_of(B, L)
    words = words_of(r) if whole_word else None
    out, labels, wrong = T.mlm_ref(r.rows, r.plan, words, seed=SEED, mask_id=WR.MASK_ID, vocab_size=WR.VOCAB, ignore_index=WR.IGN,
                                   **WR.mlm_thresholds())
    assert not wrong
    a, b = WR.band(B, L)
    tw = None if words is None else t(words)
    band_out, band_labels = WR.mlm_band(t(r.rows), t(r.plan), a, b, seed=SEED, words=tw)
    assert np.array_equal(band_out, out[a:b]) and np.array_equal(band_labels, labels[a:b])
    kw = dict(words=tw, word_len=3 if whole_word else 1, slice_rows=300)
    ids, plan, out, labels = t(r.rows), t(r.plan), t(out), t(labels)
    n_elig, n_sel, n_mask, n_rand = WR.mlm_invariants(ids, plan, out, labels, B, **kw)
    assert n_elig > 15 * r.n and n_sel > n_mask > n_rand > 0
    if whole_word:
        assert not (labels.numpy()[r.rows != out.numpy()] == WR.IGN).any()
    for breakage in (lambda x: wrapped(x, r.k), unwritten):
        with pytest.raises(AssertionError):
            WR.mlm_invariants(ids, plan, breakage(out), breakage(labels), B, **kw)
    # one element past the boundary: a selected column that holds something else, a changed column that is not selected
    row = r.k + 1
    col = int(np.nonzero(labels[row].numpy() != WR.IGN)[0][0]) if (labels[row] != WR.IGN).any() else None
    bad = out.clone()
    bad[row, 1] = 7777 if col is None else bad[row, 1]
    if col is not None:
        bad[row, col] = 7777  # (not the id, not the mask id, not below the vocabulary's size)
    fails_at(lambda: WR.mlm_invariants(ids, plan, bad, labels, B, **kw), row * L + (1 if col is None else col), B)
    bad = labels.clone()
    bad[r.n - 1, 0] = WR.BOS  # bos "selected"
    fails_at(lambda: WR.mlm_invariants(ids, plan, out, bad, B, **kw), (r.n - 1) * L, B)
    # the totals are a check of their own: a result that selects nothing passes every element and fails them
    with pytest.raises(AssertionError, match="selected columns"):
        WR.mlm_invariants(ids, plan, ids, torch.full_like(ids, WR.IGN), B, **kw)
    with pytest.raises(AssertionError, match="off"):
        WR.within_six_sigma(150 + 70, 1000, 0.15, "x")
    WR.within_six_sigma(150 + 60, 1000, 0.15, "x")


@pytest.mark.parametrize("B,L", CASES)
def test_span_band_and_invariants(B, L):
    r = rows_of(B, L)
    res = span_ref.span_corrupt_ref(r.rows, r.mask, r.plan, seed=SEED, sentinel_first=WR.SENT_FIRST, n_sentinels=WR.N_SENT,
                                    target_eos_id=WR.EOS, decoder_start_id=WR.DEC_START, pad_id=WR.PAD, ignore_index=WR.IGN,
                                    **span_ref.thresholds(0.15))
    assert not res[6]
    a, b = WR.band(B, L)
    for got, want in zip(WR.span_band(t(r.rows), t(r.mask), t(r.plan), a, b, seed=SEED), res):
        assert np.array_equal(got, want[a:b])
    out, out_mask, labels, in_len, tgt_len, dec = (t(x) for x in res[:6])
    mask = t(r.mask)
    WR.span_invariants(mask, out, out_mask, labels, in_len, tgt_len, dec, B, slice_rows=300)
    assert int((tgt_len > 1).sum()) > r.n // 2  # (most rows have noise)
    outs = [out, out_mask, labels, in_len, tgt_len, dec]
    for breakage in (lambda x: wrapped(x, r.k), unwritten):
        with pytest.raises(AssertionError):
            WR.span_invariants(mask, *[breakage(x) for x in outs], B, slice_rows=300)
    for i in range(6):  # and each output alone
        for breakage in (lambda x: wrapped(x, r.k), unwritten):
            broken = list(outs)
            broken[i] = breakage(outs[i])
            with pytest.raises(AssertionError):
                WR.span_invariants(mask, *broken, B, slice_rows=300)
    bad = in_len.clone()
    bad[r.k + 2] -= 1
    fails_at(lambda: WR.span_invariants(mask, out, out_mask, labels, bad, tgt_len, dec, B, slice_rows=300), (r.k + 2) * L, B)
    bad = labels.clone()
    bad[r.k + 1, 0] = WR.IGN  # (every row's target holds its eos at the least)
    fails_at(lambda: WR.span_invariants(mask, out, out_mask, bad, in_len, tgt_len, dec, B, slice_rows=300), (r.k + 1) * L, B)


# ---- the packed stream ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", CASES)
def test_packed_stream_sync_points_and_band(B, L):
    s = WR.packed_stream(B, L, sync_every=64, extra=8 * L)
    assert s.total > B + 8 * L and s.n_docs % 64 and (s.lens >= L).any() and (s.lens == 0).any()
    assert s.sync == list(range(0, s.n_docs - 777 + 1, 64)) and len(s.sync) > 8 and all(s.start(d) % L == 0 for d in s.sync)
    d0, d1, row0, row1 = s.band(B)
    assert d1 - d0 == 64 and row0 * L == s.start(d0) <= B < s.start(d1) == row1 * L and row1 > row0
    ids = WR.draw_ids(s.n_ids, lo=1000, hi=50000).numpy()
    c4, c16 = WR.channel_values(0, s.n_ids)
    t4, t16 = WR.channel_values(0, s.n_ids, "cpu")
    assert np.array_equal(t4.numpy(), c4) and np.array_equal(t16.numpy(), c16) and c4.dtype == np.int32 and c16.shape == (s.n_ids, 2)
    assert int(WR.channel_values(2 ** 32 + 5, 2 ** 32 + 6)[0][0]) == 5 and WR.channel_values(2 ** 32 + 5, 2 ** 32 + 6)[1].tolist() == [[2 ** 32 + 5, -2 ** 32 - 6]]
    whole = WR.packed_rows_ref(s, ids, 0, s.n_docs, flush=True)  # everything in one add, then the flush
    assert whole["input_ids"].shape == (s.total // L + 1, L)
    band = WR.packed_rows_ref(s, ids[s.offs[d0]:s.offs[d1]], d0, d1)
    dt, rowt = s.tail()
    tail = WR.packed_rows_ref(s, ids[s.offs[dt]:], dt, s.n_docs, flush=True)
    assert rowt + len(tail["input_ids"]) == len(whole["input_ids"])
    for part, first in ((band, row0), (tail, rowt)):
        n = len(part["input_ids"])
        for k in ("input_ids", "position_ids", "segment_ids"):
            assert np.array_equal(part[k], whole[k][first:first + n]), k
        for c in range(2):
            assert np.array_equal(part["channels"][c], whole["channels"][c][first:first + n])
    assert n == row1 - row0 or first == rowt
    # the checkers
    got = {k: t(whole[k]) for k in ("input_ids", "position_ids", "segment_ids")}
    got.update(c4=t(whole["channels"][0]), c16=t(whole["channels"][1]))
    WR.assert_packed_band(got, band, row0, B, "band")
    WR.assert_packed_band(got, tail, rowt, B, "tail")
    row = B // L + 1
    assert row0 <= row < row1
    for name, per in (("input_ids", L), ("position_ids", L), ("segment_ids", L), ("c4", L), ("c16", 2 * L)):
        bad = dict(got)
        bad[name] = got[name].clone()
        bad[name].view(-1)[row * per + 5] += 1
        fails_at(lambda: WR.assert_packed_band(bad, band, row0, B, "band"), row * per + 5, B)
    parts = [{k: v[:-1] for k, v in got.items()}, {k: v[-1:] for k, v in got.items()}]
    sums = (int(ids.sum(dtype=np.int64)), s.n_docs, s.n_ids)
    WR.packed_totals(parts, *sums)
    for breakage in (lambda x: wrapped(x, row), unwritten):
        broken = [{k: breakage(v) for k, v in parts[0].items()}, parts[1]]
        with pytest.raises(AssertionError):
            WR.packed_totals(broken, *sums)
    with pytest.raises(AssertionError):  # a flushed row that is all padding
        WR.packed_totals([parts[0], {k: torch.zeros_like(v) for k, v in parts[1].items()}], *sums)


# ---- copies of a block --------------------------------------------------------------------------------------------------
LO, HI = BOUNDARIES


def test_chat_block_and_its_copies():
    b = WR.chat_block(LO, HI, around=20000, room=4000)
    assert b.n_out % 2 == 1 and b.n_out >= 20000 and b.p_lo == LO % b.n_out and b.p_hi == HI % b.n_out
    WR.check_chat_layout(b)
    moved = WR.ChatBlock([[(2, 1)]] + [[(r, n) for r, n in zip(b.roles[b.conv[i]:b.conv[i + 1]].tolist(),
                                                                    np.diff(b.offsets)[b.conv[i]:b.conv[i + 1]].tolist())]
                                          for i in range(b.n_conv)], 1, LO + 0, HI + 0)
    moved.p_lo, moved.p_hi = b.p_lo, b.p_hi  # (the same places in a block that begins three elements later)
    with pytest.raises(AssertionError):
        WR.check_chat_layout(moved)
    assert (np.diff(b.offsets) == 0).sum() > 10 and set(b.roles.tolist()) == {0, 1, 2} and (np.diff(b.conv) == 0).any()
    for B in BOUNDARIES:
        R = W.copies_cross(min(b.n_ids, b.n_out), B, extra=2 ** 12)
        assert R * b.n_ids > B and (R - 1) * b.n_out < B + 2 ** 13
        ref = chat_ref.render(WR.CHAT_TPL, np.tile(b.ids, R), W.repeated_offsets(b.offsets, b.n_ids, R), np.tile(b.roles, R),
                              W.repeated_offsets(b.conv, b.n_turns, R), loss_roles=WR.CHAT_LOSS, ignore_index=WR.IGN)
        assert ref["err"] == 0
        p = B % b.n_out
        r = B // b.n_out
        assert ref["out_offsets"][np.searchsorted(ref["out_offsets"], B)] == B and ref["out_ids"][B] == WR.BOS  # a bos AT the boundary
        for k in ("out_ids", "labels", "turn_ids"):
            WR.assert_copies(t(ref[k]), b.ref[k], R, 0, B, k, slice_elems=50000)
            bad = t(ref[k]).clone()
            bad[B + 7] += 1
            fails_at(lambda: WR.assert_copies(bad, b.ref[k], R, 0, B, k, slice_elems=50000), r * b.n_out + p + 7, B)
        WR.assert_copies(t(ref["source"]), b.ref["source"], R, b.n_ids, B, "source", slice_elems=50000)
        bad = t(ref["source"]).clone()
        bad[B + 7] -= b.n_ids  # (the copy in front: what a wrapped input index gives)
        fails_at(lambda: WR.assert_copies(bad, b.ref["source"], R, b.n_ids, B, "source", slice_elems=50000), B + 7, B)
        with pytest.raises(AssertionError):  # a source that was not moved at all
            WR.assert_copies(t(np.tile(b.ref["source"], R)), b.ref["source"], R, b.n_ids, B, "source")
        oo = t(ref["out_offsets"])
        WR.assert_copy_offsets(oo, b.ref["out_offsets"], R, B, "out_offsets")
        bad = oo.clone()
        bad[-1] += 1
        with pytest.raises(AssertionError, match="total"):
            WR.assert_copy_offsets(bad, b.ref["out_offsets"], R, B, "out_offsets")
        bad = oo.clone()
        bad[r * b.n_conv + 3] += 1
        with pytest.raises(AssertionError, match="copy %d, element 3 " % r):
            WR.assert_copy_offsets(bad, b.ref["out_offsets"], R, B, "out_offsets")


def test_fim_block_and_its_copies():
    b = WR.fim_block(LO, HI, around=20000, room=4000)
    assert b.n_out % 2 == 1 and b.p_lo == LO % b.n_out and b.p_hi == HI % b.n_out
    WR.check_fim_layout(b)
    keep = b.p_lo
    b.p_lo += 1
    with pytest.raises(AssertionError):
        WR.check_fim_layout(b)
    b.p_lo = keep
    assert set(b.kinds.tolist()) == {0, 1, 2} and (np.diff(b.offsets) == 0).sum() > 10
    for B in BOUNDARIES:
        R = W.copies_cross(min(b.n_ids, b.n_out), B, extra=2 ** 12)
        offs = W.repeated_offsets(b.offsets, b.n_ids, R)
        ref = fim_ref.render(np.tile(b.ids, R), fim_ref.plan_pieces(offs), np.tile(b.kinds, R), pre=WR.PRE, suf=WR.SUF, mid=WR.MID,
                             end=WR.END, loss_parts=fim_ref.LOSS_MIDDLE, ignore_index=WR.IGN)
        for k in ("out_ids", "labels", "parts"):
            WR.assert_copies(t(ref[k]), b.ref[k], R, 0, B, k)
        assert ref["parts"][B] == fim_ref.PART_SUFFIX and ref["out_ids"][B - 2] == WR.SUF
        WR.assert_copies(t(ref["source"]), b.ref["source"], R, b.n_ids, B, "source")
        WR.assert_copy_offsets(t(ref["out_offsets"]), b.ref["out_offsets"], R, B, "out_offsets")
        bad = t(ref["parts"]).clone()
        bad[B] = fim_ref.PART_MIDDLE
        fails_at(lambda: WR.assert_copies(bad, b.ref["parts"], R, 0, B, "parts"), B, B)


# ---- fill-in-the-middle at token level ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BOUNDARIES)
def test_fim_band_and_totals(B):
    lens, offs = WR.fim_docs(B, extra=2 ** 12)
    n_docs, n_ids = len(lens), int(offs[-1])
    assert n_ids >= B + 2 ** 12 and (lens == 0).any() and (lens >= 3000).any()
    ids = WR.draw_ids(n_ids, lo=1000, hi=50000)
    whole = fim_ref.fim_tokens(ids.numpy(), offs, seed=WR.FIM_SEED, fim_below=WR.FIM_FB, spm_below=WR.FIM_SB, pre=WR.PRE, suf=WR.SUF,
                               mid=WR.MID, end=WR.END, loss_parts=fim_ref.LOSS_MIDDLE, ignore_index=WR.IGN)
    assert set(whole["kinds"].tolist()) == {0, 1, 2}
    got = {k: t(v) for k, v in whole.items()}
    d = int(np.searchsorted(offs, B, side="right")) - 1
    d0, d1 = max(0, d - 64), min(n_docs, d + 64)
    want = WR.fim_band(ids.numpy()[offs[d0]:offs[d1]], offs, d0, d1)
    assert want["plan"][:, 0].max() >= B > want["plan"][:, 0].min() and want["source"].max() > B
    WR.assert_fim_band(got, want, d0, d1, B)
    o = int(whole["out_offsets"][d + 1])
    for k in ("out_ids", "labels", "parts", "source"):
        bad = dict(got)
        bad[k] = got[k].clone()
        bad[k][o + 1] += 1
        with pytest.raises(AssertionError, match="%s at output position %d " % (k, o + 1)):
            WR.assert_fim_band(bad, want, d0, d1, B)
    for k, match in (("kinds", "kinds of document %d" % (d + 1)), ("plan", "plan of document %d" % (d + 1)), ("out_offsets", "out_offsets of document %d" % (d + 1))):
        bad = dict(got)
        bad[k] = got[k].clone()
        bad[k][d + 1] += 1
        with pytest.raises(AssertionError, match=match):
            WR.assert_fim_band(bad, want, d0, d1, B)
    n_moved = WR.fim_totals(got, t(offs), ids, n_ids, slice_elems=5000)
    assert n_moved == int((whole["kinds"] != 0).sum()) > n_docs // 3
    total = len(whole["out_ids"])
    bad = dict(got)
    bad["out_ids"] = got["out_ids"].clone()
    bad["out_ids"][total // 2:] = got["out_ids"][:total - total // 2]  # the second half a copy of the first
    with pytest.raises(AssertionError, match="sum of out_ids"):
        WR.fim_totals(bad, t(offs), ids, n_ids)
    bad = dict(got)
    bad["out_offsets"] = got["out_offsets"].clone()
    bad["out_offsets"][n_docs // 2:] -= 4
    with pytest.raises(AssertionError, match="out_offsets"):
        WR.fim_totals(bad, t(offs), ids, n_ids)


def test_guard_bands():
    x, store = WR.guarded(100, torch.int32, "cpu")
    x.fill_(5)
    assert WR.untouched(store, 100) and store.numel() == 228
    store[63] = 0
    assert not WR.untouched(store, 100)
    store[63], store[164] = WR.GUARD_VALUE, 0
    assert not WR.untouched(store, 100)
