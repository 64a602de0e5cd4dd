"""Span corruption without a GPU: the numpy restatement of tests/span_ref.py on rows worked by hand from printed draws,
the round trip from its outputs back to the rows, the density of the merged process, every argument check of
corrupt_spans / batch_encode_span_corruption that comes before a device call, what the C call refuses before it looks
for a device, and the draws of csrc/hutk_philox.h compiled for the host.  The kernel is compared with the restatement in
tests/test_gpu_span_corruption.py."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import span_ref as S
import targets_ref as T

import hutoken_amd
from hutoken_amd import _capi

CORRUPT, BATCH = hutoken_amd.corrupt_spans, hutoken_amd.batch_encode_span_corruption  # (what span_ref.py restates: nothing here runs without them)
I = -100  # the ignore index of the worked rows
ONE = 2**32
# The worked rows draw with four lengths of equal weight and a start probability of 1/4, so that a draw reads off its two
# top bits: a column starts a span iff u0 >> 30 == 0, of the length 1 + (u1 >> 30).
QUARTERS = dict(start_below=ONE // 4, len_below=[ONE // 4, ONE // 2, 3 * (ONE // 4), ONE])
WORKED = dict(QUARTERS, sentinel_first=99, sentinel_step=-1, target_eos_id=7, decoder_start_id=5)
# the draws of row 0, columns 0 .. 11, as printed: S where the column would start a span; the length it would draw
DRAWS = {3: ("....S...S..S", "344414241131"),
         5: ("...S.S..S...", "444222212322"),
         14: (".S.S.S......", "444122314222"),
         21: (".S...S......", "311113314114"),
         25: ("...SS...S...", "422331443111")}


def rows(*r):
    return np.array(r, dtype=np.int64)


PAD_RIGHT = dict(ids=rows([1, 10, 11, 12, 13, 14, 15, 16, 17, 2, 0, 0]), mask=rows([1] * 10 + [0, 0]), plan=rows([0, 0, 0, 8, 1, 0, 0, 9]))
PAD_LEFT = dict(ids=rows([0, 0, 1, 10, 11, 12, 13, 14, 15, 16, 17, 2]), mask=rows([0, 0] + [1] * 10), plan=rows([0, 0, 0, 8, 3, 0, 0, 11]))
PAIR = dict(ids=rows([1, 10, 11, 12, 3, 20, 21, 22, 23, 2, 0, 0]), mask=rows([1] * 10 + [0, 0]), plan=rows([0, 0, 0, 3, 1, 0, 4, 5]))


def corrupt(case, seed, **kw):
    """-> (corrupted row, its length, target row, its length, decoder row) of the one row of a worked case"""
    out, out_mask, labels, in_len, tgt_len, dec, wrong = S.span_corrupt_ref(case["ids"], case["mask"], case["plan"], seed=seed,
                                                                            **dict(WORKED, **kw))
    assert not wrong
    assert out_mask[0].tolist() == [1] * int(in_len[0]) + [0] * (12 - int(in_len[0]))
    return out[0].tolist(), int(in_len[0]), labels[0].tolist(), int(tgt_len[0]), None if dec is None else dec[0].tolist()


def test_the_printed_draws():
    for seed, (starts, lengths) in DRAWS.items():
        u0, u1, _u2, _u3 = T.draw(seed, 0, np.arange(12), S.SPAN)
        assert "".join("S" if int(x) >> 30 == 0 else "." for x in u0) == starts
        assert "".join(str(1 + (int(x) >> 30)) for x in u1) == lengths
    assert S.SPAN == 3 and len({int(T.draw(9, 4, 2, purpose)[0]) for purpose in (T.COLUMN, T.WORD_A, T.WORD_B, S.SPAN)}) == 4


def test_two_runs_of_a_worked_row():
    """Seed 21 on [bos 10 .. 17 eos pad pad]: column 1 starts a span of 1, column 5 one of 3 (columns 5, 6, 7)."""
    out, n, target, t, dec = corrupt(PAD_RIGHT, 21)
    assert (out, n) == ([1, 99, 11, 12, 13, 98, 17, 2, 0, 0, 0, 0], 8)
    assert (target, t) == ([99, 10, 98, 14, 15, 16, 7, I, I, I, I, I], 7)
    assert dec == [5, 99, 10, 98, 14, 15, 16, 7, 0, 0, 0, 0]
    # one sentinel: the second run stays text
    out, n, target, t, dec = corrupt(PAD_RIGHT, 21, n_sentinels=1)
    assert (out, n) == ([1, 99, 11, 12, 13, 14, 15, 16, 17, 2, 0, 0], 10)
    assert (target, t) == ([99, 10, 7, I, I, I, I, I, I, I, I, I], 3)
    out, n, target, t, dec = corrupt(PAD_RIGHT, 21, n_sentinels=0)
    assert (out, n) == (PAD_RIGHT["ids"][0].tolist(), 10) and (target, t) == ([7] + [I] * 11, 1) and dec == [5, 7] + [0] * 10
    # sentinels that count up; no eos; no decoder row; another fill
    out, n, target, t, dec = corrupt(PAD_RIGHT, 21, sentinel_step=1, target_eos_id=None, decoder_start_id=None, pad_id=-1, ignore_index=-7)
    assert (out, n) == ([1, 99, 11, 12, 13, 100, 17, 2, -1, -1, -1, -1], 8)
    assert (target, t) == ([99, 10, 100, 14, 15, 16, -7, -7, -7, -7, -7, -7], 6) and dec is None
    # nothing starts; the row number is part of the draw
    assert corrupt(PAD_RIGHT, 21, start_below=0)[:2] == (PAD_RIGHT["ids"][0].tolist(), 10)
    other = S.span_corrupt_ref(PAD_RIGHT["ids"], PAD_RIGHT["mask"], PAD_RIGHT["plan"], seed=21, first_row=1, **WORKED)
    assert other[0][0].tolist() != out


def test_target_truncation():
    for L_tgt, want, want_dec in ((4, [99, 10, 98, 14], [5, 99, 10, 98]), (6, [99, 10, 98, 14, 15, 16], [5, 99, 10, 98, 14, 15]),
                                  (7, [99, 10, 98, 14, 15, 16, 7], [5, 99, 10, 98, 14, 15, 16]), (1, [99], [5]),
                                  (9, [99, 10, 98, 14, 15, 16, 7, I, I], [5, 99, 10, 98, 14, 15, 16, 7, 0])):
        out, n, target, t, dec = corrupt(PAD_RIGHT, 21, max_target_len=L_tgt)
        assert (target, t, dec) == (want, 7, want_dec)  # the length is the untruncated one
        assert (out, n) == ([1, 99, 11, 12, 13, 98, 17, 2, 0, 0, 0, 0], 8)


def test_runs_that_overlap_and_touch_merge():
    """Seed 14: column 1 starts a span of 4 (1 .. 4), column 3 one of 1 inside it, column 5 one of 2 (5, 6) that touches it:
    one run of columns 1 .. 6."""
    out, n, target, t, _dec = corrupt(PAD_RIGHT, 14)
    assert (out, n) == ([1, 99, 16, 17, 2, 0, 0, 0, 0, 0, 0, 0], 5)
    assert (target, t) == ([99, 10, 11, 12, 13, 14, 15, 7, I, I, I, I], 8)


def test_a_run_ends_with_its_side():
    """[bos 10 11 12 sep 20 21 22 23 eos pad pad].  Seed 25: column 3 starts a span of 3 that would cover the separator and
    column 5 of B: it ends with A, at column 4; column 4 is no text and starts nothing; column 8 starts a span of 3 that
    ends with B, in front of eos."""
    out, n, target, t, _dec = corrupt(PAIR, 25)
    assert (out, n) == ([1, 10, 11, 99, 3, 20, 21, 22, 98, 2, 0, 0], 10)
    assert (target, t) == ([99, 12, 98, 23, 7, I, I, I, I, I, I, I], 5)
    # seed 5: column 3 a span of 2 (cut to 1), column 5 one of 2, column 8 one of 2 (cut to 1): the numbering runs on from A into B
    out, n, target, t, _dec = corrupt(PAIR, 5)
    assert (out, n) == ([1, 10, 11, 99, 3, 98, 22, 97, 2, 0, 0, 0], 9)
    assert (target, t) == ([99, 12, 98, 20, 21, 97, 23, 7, I, I, I, I], 8)
    out, n, target, t, _dec = corrupt(PAIR, 5, sides=T.SIDE_A)
    assert (out, n) == ([1, 10, 11, 99, 3, 20, 21, 22, 23, 2, 0, 0], 10) and (target[:4], t) == ([99, 12, 7, I], 3)
    out, n, target, t, _dec = corrupt(PAIR, 5, sides=T.SIDE_B)
    assert (out, n) == ([1, 10, 11, 12, 3, 99, 22, 98, 2, 0, 0, 0], 9) and (target[:7], t) == ([99, 20, 21, 98, 23, 7, I], 6)
    # a mask byte of 0 inside a side: the column is neither kept nor noise, and it ends a run
    holed = dict(PAIR, mask=rows([1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0]))
    out, n, target, t, _dec = corrupt(holed, 5)
    assert (out, n) == ([1, 10, 11, 99, 3, 98, 22, 97, 2, 0, 0, 0], 9) and (target[:8], t) == ([99, 12, 98, 20, 97, 23, 7, I], 7)


def test_a_left_padded_row_comes_out_right_padded():
    """[pad pad bos 10 .. 17 eos].  Seed 3: columns 4 and 8 start a span of 1 each (the ids 11 and 15); column 11 is eos
    and starts nothing."""
    out, n, target, t, dec = corrupt(PAD_LEFT, 3)
    assert (out, n) == ([1, 10, 99, 12, 13, 14, 98, 16, 17, 2, 0, 0], 10)
    assert (target, t) == ([99, 11, 98, 15, 7, I, I, I, I, I, I, I], 5)
    assert dec == [5, 99, 11, 98, 15, 7, 0, 0, 0, 0, 0, 0]


def test_hostile_plans_by_the_restatement():
    ids, mask = rows([5, 6, 7, 8, 9, 10]), rows([1] * 6)
    always = dict(seed=1, start_below=ONE, len_below=[ONE], sentinel_first=99)
    # A begins in front of the row (clipped to columns 0, 1); B claims column 1 too (it is A's) and 2, 3: one run of four
    out, _m, labels, in_len, tgt_len, _dec, wrong = S.span_corrupt_ref(ids, mask, rows([0, 0, 0, 4, -2, 0, 3, 1]), **always)
    assert wrong and out[0].tolist() == [99, 9, 10, 0, 0, 0] and labels[0].tolist() == [99, 5, 6, 7, 8, I]
    for plan in (rows([0, 0, 0, -3, 1, 0, -1, 2]), rows([0, 0, 0, 2, 6, 0, 2, 2**62]), rows([0, 0, 0, 2**63 - 1, -2**62, 0, 0, 0])):
        out, _m, labels, in_len, tgt_len, _dec, wrong = S.span_corrupt_ref(ids, mask, plan, **always)
        assert wrong and out[0].tolist() == ids[0].tolist() and (labels == I).all() and tgt_len[0] == 0


# ---- the round trip -----------------------------------------------------------------------------------------------------
def restored(out, in_len, labels, tgt_len, sentinels, eos):
    """Every sentinel of a corrupted row replaced by the ids that follow it in the target -> the row it was made from"""
    target = labels[:tgt_len].tolist()
    if eos is not None:
        assert target[-1] == eos
        target = target[:-1]
    spans, key = {}, None
    for x in target:
        if x in sentinels:
            key = x
            assert key not in spans
            spans[key] = []
        else:
            spans[key].append(x)
    row = []
    for x in out[:in_len].tolist():
        row += spans.pop(x) if x in sentinels else [x]
    assert not spans
    return row


def random_rows(n, L, rng, pairs=True):
    """n rows of every kind the collation makes, made here: [bos] A [sep B] [eos] padded on either side -> ids, mask, plan"""
    ids = rng.integers(100, 50000, size=(n, L)).astype(np.int64)
    mask, plan = np.zeros((n, L), dtype=np.uint8), np.zeros((n, 8), dtype=np.int64)
    for r in range(n):
        bos, eos, sep = (int(x) for x in rng.integers(0, 2, size=3))
        sep = sep if pairs else 0
        room = L - bos - eos - sep
        ka = int(rng.integers(0, room + 1))
        kb = int(rng.integers(0, room - ka + 1)) if sep else 0
        length = bos + ka + sep + kb + eos
        first = (L - length) * int(rng.integers(0, 2))  # padded on the right or on the left
        mask[r, first:first + length] = 1
        ids[r, :first], ids[r, first + length:] = 0, 0
        plan[r] = [r, 0, 0, ka, first + bos, 0, kb, first + bos + ka + sep]
    return ids, mask, plan


def test_round_trip_of_200_random_rows():
    rng = np.random.default_rng(1)
    L = 96
    ids, mask, plan = random_rows(200, L, rng)
    sentinels = set(range(60000 - 99, 60001))
    for seed, density, eos in ((1, 0.15, 7), (2, 0.5, None), (3, 0.9, 7)):
        res = S.span_corrupt_ref(ids, mask, plan, seed=seed, sentinel_first=60000, target_eos_id=eos, max_target_len=2 * L + 1,
                                 **S.thresholds(density))
        out, out_mask, labels, in_len, tgt_len, _dec, wrong = res
        assert not wrong and (tgt_len > (eos is not None)).sum() > 150
        for r in range(len(ids)):
            assert restored(out[r], in_len[r], labels[r], tgt_len[r], sentinels, eos) == ids[r][mask[r] != 0].tolist(), (seed, r)
            assert (out[r, in_len[r]:] == 0).all() and out_mask[r].tolist() == [1] * in_len[r] + [0] * (L - in_len[r])


# ---- the density --------------------------------------------------------------------------------------------------------
def test_density_of_the_merged_process():
    """2048 rows of 512 text columns.  The noise indicators correlate over at most max_span columns, so the variance of
    their sum is at most 2 * max_span * d * N; a side's first max_span - 1 columns see fewer predecessors."""
    n, L, max_span = 2048, 512, 10
    mask = np.ones((n, L), dtype=np.uint8)
    plan = np.zeros((n, 8), dtype=np.int64)
    plan[:, 3], plan[:, 7] = L, L
    for d in (0.15, 0.5):
        noise, _eligible, wrong = S.noise_columns(mask, plan, seed=20, **S.thresholds(d, 3.0, max_span))
        fraction = float(noise.mean())
        bound = 5 * (2 * max_span * d / (n * L)) ** 0.5 + (max_span - 1) / L
        print("density", d, "fraction", fraction, "bound", bound)
        assert not wrong and abs(fraction - d) <= bound
    assert round(5 * (2 * max_span * 0.15 / (n * L)) ** 0.5 + (max_span - 1) / L, 3) == 0.026


def test_tables_and_start_probabilities():
    """tests/span_ref.py and the package do the same arithmetic: a GPU test hands both the same integers."""
    for kw in (dict(), dict(mean_span_length=1), dict(mean_span_length=5.5, max_span_length=32), dict(max_span_length=1),
               dict(span_length_probs=[1.0]), dict(span_length_probs=[0.0] * 31 + [1.0]), dict(span_length_probs=[0.5, 0.25, 0.25, 0, 0])):
        full = dict(dict(mean_span_length=3.0, max_span_length=10, span_length_probs=None), **kw)
        len_below, tail = hutoken_amd._span_length_table(**full)
        assert (len_below, tail) == S.length_table(**full)
        assert len_below[-1] == ONE and all(0 <= a <= b for a, b in zip(len_below, len_below[1:])) and tail[0] == 1.0
        for d in (0.0, 0.01, 0.15, 0.5):
            p = hutoken_amd._span_start_probability(d, tail)
            assert p == S.start_probability(d, tail) and abs(S.density(p, tail) - d) < 1e-12
    assert S.length_table()[0][:3] == [int(ONE / 3), int((1 / 3 + 2 / 9) * ONE), int((1 / 3 + 2 / 9 + 4 / 27) * ONE)]
    assert S.thresholds(1.0, span_length_probs=[1.0]) == dict(start_below=ONE, len_below=[ONE])
    assert S.thresholds(0.0)["start_below"] == 0
    assert S.length_table(span_length_probs=[0.0] * 31 + [1.0])[0] == [0] * 31 + [ONE]


# ---- the Python surface: argument checks come before any device call ------------------------------------------------
def test_names_are_exported():
    for name in ("corrupt_spans", "batch_encode_span_corruption"):
        assert name in hutoken_amd.__all__ and callable(getattr(hutoken_amd, name)) and name in hutoken_amd.__doc__
    assert "hutk_rows_span_corrupt_device" in _capi.EXPORTS
    fn = _capi.load().hutk_rows_span_corrupt_device
    assert fn.argtypes is not None and len(fn.argtypes) == 27


def host_rows(n=2, L=4, dtype=None):
    import torch
    return torch.zeros((n, L), dtype=dtype or torch.int32), torch.ones((n, L), dtype=torch.uint8), torch.zeros((n, 8), dtype=torch.int64)


def test_corrupt_spans_argument_checks():
    import torch
    ids, mask, plan = host_rows()
    ok = dict(sentinel_first=32099, seed=0)
    call = CORRUPT
    with pytest.raises(TypeError, match="seed"):
        call(ids, mask, plan, sentinel_first=5)  # no default
    with pytest.raises(TypeError, match="sentinel_first"):
        call(ids, mask, plan, seed=5)
    for bad in ([[1, 2]], None, np.zeros((2, 4), dtype=np.int32)):
        with pytest.raises(TypeError, match="input_ids"):
            call(bad, mask, plan, **ok)
    for bad in (torch.int16, torch.float32, torch.uint8):
        with pytest.raises(TypeError, match="input_ids"):
            call(ids.to(bad), mask, plan, **ok)
    for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros((2, 0), dtype=torch.int32), torch.zeros((2, 8), dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match="input_ids"):
            call(bad, mask, plan, **ok)
    for bad in (None, [[1] * 4] * 2):
        with pytest.raises(TypeError, match="attention_mask"):
            call(ids, bad, plan, **ok)
    for bad in (torch.int32, torch.bool, torch.int8):
        with pytest.raises(TypeError, match="attention_mask"):
            call(ids, mask.to(bad), plan, **ok)
    for bad in (torch.ones((2, 5), dtype=torch.uint8), torch.ones(8, dtype=torch.uint8), torch.ones((2, 8), dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError, match="attention_mask"):
            call(ids, bad, plan, **ok)
    with pytest.raises(TypeError, match="row_plan"):
        call(ids, mask, plan.to(torch.int32), **ok)
    for bad in (torch.zeros((3, 8), dtype=torch.int64), torch.zeros((2, 7), dtype=torch.int64)):
        with pytest.raises(ValueError, match="row_plan"):
            call(ids, mask, bad, **ok)
    for bad in (True, 1.0, "1", None):
        with pytest.raises(TypeError, match="seed"):
            call(ids, mask, plan, sentinel_first=5, seed=bad)
        with pytest.raises(TypeError, match="sentinel_first"):
            call(ids, mask, plan, sentinel_first=bad, seed=0)
        with pytest.raises(TypeError, match="n_sentinels"):
            call(ids, mask, plan, n_sentinels=bad, **ok)
    for bad in (-1, 2**64):
        with pytest.raises(ValueError, match="seed"):
            call(ids, mask, plan, sentinel_first=5, seed=bad)
    for bad in (2, 0, -2):
        with pytest.raises(ValueError, match="sentinel_step"):
            call(ids, mask, plan, sentinel_step=bad, **ok)
    with pytest.raises(TypeError, match="sentinel_step"):
        call(ids, mask, plan, sentinel_step=1.0, **ok)
    with pytest.raises(ValueError, match="n_sentinels"):
        call(ids, mask, plan, n_sentinels=-1, **ok)
    # sentinels that leave int32: the first one, the last one counting up, the last one counting down
    for kw in (dict(sentinel_first=2**31), dict(sentinel_first=2**31 - 50, sentinel_step=1), dict(sentinel_first=-2**31 + 50),
               dict(sentinel_first=-2**31 - 1, n_sentinels=0)):
        with pytest.raises(ValueError, match="fit int32"):
            call(ids, mask, plan, seed=0, **kw)
    with pytest.raises(ValueError, match="fit int64"):
        call(ids.to(torch.int64), mask, plan, seed=0, sentinel_first=2**63 - 50, sentinel_step=1)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="noise_density"):
            call(ids, mask, plan, noise_density=bad, **ok)
    with pytest.raises(TypeError, match="noise_density"):
        call(ids, mask, plan, noise_density="0.15", **ok)
    # A density the table cannot reach.  With p = 1 every eligible column starts a span and the factor of j = 0 in
    # 1 - prod_j (1 - p * P(len > j)) is 0: every table reaches every density up to 1, so the only ones out of reach
    # are those above 1, and the bisection's own refusal is reached with a table that is none (tails below 1).
    with pytest.raises(ValueError, match="noise_density"):
        call(ids, mask, plan, noise_density=1.0 + 1e-9, **ok)
    assert hutoken_amd._span_start_probability(1.0, S.length_table()[1]) == 1.0
    with pytest.raises(ValueError, match="cannot be reached"):
        hutoken_amd._span_start_probability(0.5, [0.25, 0.125])
    for bad in ([0.5, 0.4], [0.5, 0.6], [1.0, 1e-6]):  # probabilities that do not sum to 1
        with pytest.raises(ValueError, match="sum to 1"):
            call(ids, mask, plan, span_length_probs=bad, **ok)
    with pytest.raises(ValueError, match="1 .. 32"):
        call(ids, mask, plan, span_length_probs=[1 / 33] * 33, **ok)  # 33 lengths
    with pytest.raises(ValueError, match="1 .. 32"):
        call(ids, mask, plan, span_length_probs=[], **ok)
    with pytest.raises(ValueError, match="span_length_probs"):
        call(ids, mask, plan, span_length_probs=[1.5, -0.5], **ok)
    for bad in ("0.5 0.5", 3, [0.5, "0.5"], [True, 0]):
        with pytest.raises(TypeError, match="span_length_probs"):
            call(ids, mask, plan, span_length_probs=bad, **ok)
    for bad in (0.5, 0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="mean_span_length"):
            call(ids, mask, plan, mean_span_length=bad, **ok)
    with pytest.raises(TypeError, match="mean_span_length"):
        call(ids, mask, plan, mean_span_length="3", **ok)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="max_span_length"):
            call(ids, mask, plan, max_span_length=bad, **ok)
    with pytest.raises(TypeError, match="max_span_length"):
        call(ids, mask, plan, max_span_length=10.0, **ok)
    for name in ("target_eos_id", "decoder_start_id", "pad_id"):
        with pytest.raises(TypeError, match=name):
            call(ids, mask, plan, **dict(ok, **{name: 1.0}))
        with pytest.raises(ValueError, match=name):
            call(ids, mask, plan, **dict(ok, **{name: 2**31}))
    with pytest.raises(TypeError, match="pad_id"):
        call(ids, mask, plan, pad_id=None, **ok)
    for bad in (0, -1, 2**31):
        with pytest.raises(ValueError, match="max_target_length"):
            call(ids, mask, plan, max_target_length=bad, **ok)
    with pytest.raises(TypeError, match="max_target_length"):
        call(ids, mask, plan, max_target_length=4.0, **ok)
    with pytest.raises(ValueError, match="fit int32"):
        call(ids, mask, plan, ignore_index=2**31, **ok)
    with pytest.raises(TypeError, match="ignore_index"):
        call(ids, mask, plan, ignore_index=-100.0, **ok)
    for bad in ("A", "ab", 3, None):
        with pytest.raises(ValueError, match="sides"):
            call(ids, mask, plan, sides=bad, **ok)
    # sound arguments on the host: refused for where they are, not computed there
    for kw in ({}, {"noise_density": 1.0, "span_length_probs": [1.0]}, {"noise_density": 0, "n_sentinels": 0},
               {"target_eos_id": 1, "decoder_start_id": 0, "max_target_length": 1, "sides": "b", "sentinel_step": 1},
               {"mean_span_length": 1, "max_span_length": 32, "seed": 2**64 - 1}):
        with pytest.raises(ValueError, match="on the GPU"):
            call(ids, mask, plan, **dict(ok, **kw))
        with pytest.raises(ValueError, match="on the GPU"):
            call(ids.to(torch.int64), mask, plan, **dict(ok, **kw))


def test_batch_encode_span_corruption_checks_before_it_encodes(monkeypatch):
    call = BATCH
    monkeypatch.setattr(hutoken_amd, "_ctx", None)
    with pytest.raises(TypeError, match="seed"):
        call(["a"], 8, sentinel_first=50000)
    with pytest.raises(TypeError, match="sentinel_first"):
        call(["a"], 8, seed=0)
    with pytest.raises(TypeError, match="plan"):
        call(["a"], 8, sentinel_first=50000, seed=0, return_plan=True)
    with pytest.raises(ValueError, match="sentinel_step"):
        call(["a"], 8, sentinel_first=50000, seed=0, sentinel_step=2)
    with pytest.raises(ValueError, match="noise_density"):
        call(["a"], 8, sentinel_first=50000, seed=0, noise_density=1.01)
    with pytest.raises(ValueError, match="sum to 1"):
        call(["a"], 8, sentinel_first=50000, seed=0, span_length_probs=[0.5])
    with pytest.raises(ValueError, match="sides"):
        call(["a"], 8, sentinel_first=50000, seed=0, sides="c")
    with pytest.raises(ValueError, match="fit int32"):
        call(["a"], 8, sentinel_first=2**31 + 5, seed=0)
    with pytest.raises(RuntimeError, match="initialize"):
        call(["a"], 8, sentinel_first=2**31 + 5, seed=0, dtype="int64")
    with pytest.raises(RuntimeError, match="initialize"):
        call(["a"], 8, sentinel_first=50000, seed=0)


# ---- the C ABI: what is refused before a device is looked for -------------------------------------------------------
def c_span(n_rows=0, max_len=8, width=4, start=0, table=(ONE,), n_len=None, first=100, step=-1, n_sent=10, eos=_capi.NO_TOKEN,
           dec_start=_capi.NO_TOKEN, pad=0, ignore=-100, sides=3, max_tgt=8, plan=None, ids=None, mask=None, out=None, out_mask=None,
           labels=None, dec=None, in_len=None, tgt_len=None, err=None):
    import ctypes
    arr = None if table is None else (ctypes.c_int64 * len(table))(*table)
    return _capi.load().hutk_rows_span_corrupt_device(plan, n_rows, max_len, ids, width, mask, 1234, start, arr,
                                                      (0 if table is None else len(table)) if n_len is None else n_len, first, step,
                                                      n_sent, eos, dec_start, pad, ignore, sides, max_tgt, out, out_mask, labels, dec,
                                                      in_len, tgt_len, err, None)


BUFFERS = dict(plan=0x1000, ids=0x2000, mask=0x3000, out=0x4000, out_mask=0x5000, labels=0x6000, in_len=0x7000, tgt_len=0x8000)


def test_c_abi_argument_checks_need_no_device():
    E = _capi.E_ARG
    for width in (0, 2, 16, -4):
        assert c_span(width=width) == E
    for bad in (0, -1, 2**31):
        assert c_span(max_len=bad) == E
        assert c_span(max_tgt=bad) == E
    assert "max_target_len" in _capi.last_error()
    assert c_span(n_rows=-1) == E
    for bad in (-1, ONE + 1):
        assert c_span(start=bad) == E
    assert "start_below" in _capi.last_error()
    for table in ((), None, (ONE // 33,) * 32 + (ONE,), (5, 4, ONE), (-1, ONE), (ONE + 1,), (0, ONE - 1), (ONE, ONE - 1)):
        assert c_span(table=table) == E, table
        assert "len_below" in _capi.last_error()
    assert c_span(table=(ONE,), n_len=0) == E and c_span(table=(ONE,), n_len=-1) == E
    for step in (0, 2, -2):
        assert c_span(step=step) == E
    assert "sentinel_step" in _capi.last_error()
    assert c_span(n_sent=-1) == E
    for kw in (dict(first=2**31), dict(first=-2**31 - 1), dict(first=2**31 - 5, step=1), dict(first=-2**31 + 5, step=-1),
               dict(first=2**31, n_sent=0), dict(width=8, first=2**63 - 5, step=1), dict(width=8, first=-2**63 + 5, step=-1, n_sent=2**62)):
        assert c_span(**kw) == E, kw
        assert "sentinel" in _capi.last_error()
    assert c_span(pad=2**31) == E and "pad_id" in _capi.last_error()
    assert c_span(ignore=2**31) == E and c_span(ignore=-2**31 - 1) == E and "ignore_index" in _capi.last_error()
    for sides in (0, 4, 7, -1):
        assert c_span(sides=sides) == E
    assert c_span(err=0x1002) == E
    # with rows: a NULL buffer, a misaligned one, outputs over inputs or over each other (addresses that nothing reads)
    for name in BUFFERS:
        assert c_span(n_rows=1, **dict(BUFFERS, **{name: None})) == E and "NULL" in _capi.last_error(), name
    assert c_span(n_rows=1, dec_start=5, **BUFFERS) == E and "NULL" in _capi.last_error()  # a decoder row is asked for
    for name, at in (("plan", 0x1004), ("ids", 0x2002), ("out", 0x4002), ("labels", 0x6001), ("in_len", 0x7002), ("tgt_len", 0x8001)):
        assert c_span(n_rows=1, **dict(BUFFERS, **{name: at})) == E and "aligned" in _capi.last_error(), name
    assert c_span(n_rows=1, width=8, **dict(BUFFERS, ids=0x2004)) == E and "aligned" in _capi.last_error()
    assert c_span(n_rows=1, dec_start=5, dec=0x9002, **BUFFERS) == E and "aligned" in _capi.last_error()
    for kw in (dict(out=0x2000), dict(out=0x2010), dict(out_mask=0x3004), dict(labels=0x1020), dict(labels=0x2000), dict(in_len=0x3000),
               dict(tgt_len=0x2004), dict(err=0x2008), dict(err=0x103c), dict(out_mask=0x2010)):
        assert c_span(n_rows=1, **dict(BUFFERS, **kw)) == E and "overlap an input" in _capi.last_error(), kw
    for kw in (dict(labels=0x4000), dict(labels=0x4010), dict(out_mask=0x4004), dict(tgt_len=0x7000), dict(in_len=0x6004), dict(err=0x7000),
               dict(err=0x401c)):
        assert c_span(n_rows=1, **dict(BUFFERS, **kw)) == E and "overlap each other" in _capi.last_error(), kw
    for dec in (0x2000, 0x6000, 0x6010, 0x4010):
        assert c_span(n_rows=1, dec_start=5, dec=dec, **BUFFERS) == E and "overlap" in _capi.last_error(), dec
    assert c_span(n_rows=2, **dict(BUFFERS, labels=0x4020)) == E  # the second row of the corrupted ids
    # more rows than one launch holds, or than a size in bytes: refused before the buffers are looked at or a device is
    for n_rows in (2**63 - 1, 2**63 - 3, 4 * (2**31 - 1) + 1, 2**33):
        assert c_span(n_rows=n_rows, **BUFFERS) == _capi.E_UNSUPPORTED, n_rows
    assert c_span(n_rows=2**32, max_len=2**31 - 1, width=8, **BUFFERS) == _capi.E_UNSUPPORTED  # 2^66 bytes


def test_sound_arguments_without_rows():
    """Limits that are allowed, with n_rows == 0: nothing is written and nothing launched; without a GPU the call fails
    loudly after the argument checks."""
    import torch
    want = _capi.OK if torch.cuda.is_available() else _capi.E_DEVICE
    assert c_span() == want
    assert c_span(start=ONE, table=(0,) * 31 + (ONE,), first=2**31 - 1, step=-1, n_sent=2**32, max_len=2**31 - 1, max_tgt=2**31 - 1) == want
    assert c_span(width=8, first=2**62, step=1, n_sent=2**62, pad=-2**63, ignore=2**63 - 1, sides=1, eos=1, dec_start=2) == want
    assert c_span(table=(5, 5, ONE, ONE), n_sent=0, first=-2**31, sides=2) == want
    if not torch.cuda.is_available():
        # With rows, and only where no device can be found: the call ends with HUTK_E_DEVICE before anything is launched
        # on these invented addresses.  No decoder row is asked for, so d_decoder_ids, which lies over the ids, is not
        # looked at (with real buffers: test_gpu_span_corruption.test_decoder_ids_are_not_looked_at_without_a_start_id).
        assert c_span(n_rows=1, dec=0x2000, **BUFFERS) == _capi.E_DEVICE


# ---- the generator's header, compiled for the host ----------------------------------------------------------------------
MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "hutk_philox.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 2 < argc; i += 3) {
        const hutk::Philox4 d = hutk::draw(strtoull(argv[i], nullptr, 10), strtoll(argv[i + 1], nullptr, 10),
                                           (uint32_t)strtoul(argv[i + 2], nullptr, 10), hutk::DRAW_SPAN);
        printf("%u %u %u %u\n", d.x, d.y, d.z, d.w);
    }
    return hutk::DRAW_SPAN == 3 ? 0 : 1;
}
"""


def test_host_header_draws_like_numpy(tmp_path):
    src, exe = str(tmp_path / "draws.cpp"), str(tmp_path / "draws")
    with open(src, "w") as f:
        f.write(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(H.ROOT, "hutoken_amd", "csrc"), src, "-o", exe])
    cases = [(0, 0, 0), (21, 0, 5), (1234, 399, 511), (2**64 - 1, 2**40 + 3, 2**31 - 2), (0x299f31d0a4093822, 7, 4096)]
    r = subprocess.run([exe] + [str(x) for case in cases for x in case], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert got == [tuple(int(x) for x in T.draw(seed, row, col, S.SPAN)) for seed, row, col in cases]
