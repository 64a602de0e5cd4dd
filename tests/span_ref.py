"""Span corruption in plain numpy: the definition that k_rows_span_corrupt of csrc/hutk_collate.hip is tested against
(the rule is stated in full in include/hutoken_amd.h).

Every column of every row is decided at once from the plan, the mask and the draws -- the noise by
np.maximum.accumulate over the reaches -- and the rows are then built run by run in Python lists: nothing here scans,
packs or compacts the way the kernel does.  length_table and start_probability restate the arithmetic of
hutoken_amd.corrupt_spans, so that a test hands the kernel and this file the same integers."""
import numpy as np

import targets_ref as T

SPAN = 3  # the purpose of a span draw
ONE = 2**32


def length_table(mean_span_length=3.0, max_span_length=10, span_length_probs=None):
    """-> (len_below, tail): len_below[j] = int(P(len <= j + 1) * 2**32) with the last entry 2**32; tail[j] = P(len > j)"""
    if span_length_probs is not None:
        probs = [float(x) for x in span_length_probs]
    else:
        q = 1.0 - 1.0 / float(mean_span_length)
        probs = [(1.0 - q) * q**j for j in range(max_span_length - 1)] + [q**(max_span_length - 1)]
    len_below, tail, cum = [], [], 0.0
    for x in probs:
        tail.append(min(1.0, max(0.0, 1.0 - cum)))
        cum += x
        len_below.append(min(ONE, max(int(cum * ONE), len_below[-1] if len_below else 0)))
    len_below[-1] = ONE
    return len_below, tail


def density(p, tail):
    """the probability that a column far from its side's start is noise: 1 - prod_j (1 - p * P(len > j))"""
    clear = 1.0
    for t in tail:
        clear *= 1.0 - p * t
    return 1.0 - clear


def start_probability(noise_density, tail):
    if noise_density <= 0.0:
        return 0.0
    most = density(1.0, tail)
    if noise_density > most + 1e-12:
        raise ValueError("unreachable")
    if noise_density >= most:
        return 1.0
    lo, hi = 0.0, 1.0
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if density(mid, tail) < noise_density:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def thresholds(noise_density=0.15, mean_span_length=3.0, max_span_length=10, span_length_probs=None):
    """the two integers of a corrupt_spans call -> dict(start_below=, len_below=)"""
    len_below, tail = length_table(mean_span_length, max_span_length, span_length_probs)
    return dict(start_below=int(start_probability(float(noise_density), tail) * ONE), len_below=len_below)


def noise_columns(mask, plan, *, seed, start_below, len_below, sides=T.SIDE_A | T.SIDE_B, first_row=0):
    """-> (noise0 bool [n_rows, L]: the noise in front of the n_sentinels filter, eligible, wrong)"""
    mask, plan = np.asarray(mask), np.asarray(plan).reshape(-1, 8)
    n_rows, L = mask.shape
    in_a, in_b, _end_b, wrong = T.plan_sides(plan, L)
    side_end = np.zeros((n_rows, L), dtype=np.int64)
    for r, (_item, _start, _sa, ka, ca, _sb, kb, cb) in enumerate(plan.tolist()):
        side_end[r, in_a[r]] = T.clip_side(ca, ka, L)[1]
        side_end[r, in_b[r]] = T.clip_side(cb, kb, L)[1]
    eligible = np.zeros((n_rows, L), dtype=bool)
    if sides & T.SIDE_A:
        eligible |= in_a
    if sides & T.SIDE_B:
        eligible |= in_b
    eligible &= mask != 0
    r, c = np.nonzero(eligible)
    u0, u1, _u2, _u3 = T.draw(seed, first_row + r, c, SPAN)
    length = np.ones(len(r), dtype=np.int64)
    for t in len_below[:-1]:
        length += u1 >= np.uint64(t)
    reach = np.zeros((n_rows, L), dtype=np.int64)
    reach[r, c] = np.where(u0 < np.uint64(start_below), np.minimum(c + length, side_end[r, c]), 0)
    covered = np.maximum.accumulate(reach, axis=1) > np.arange(L)[None, :]
    return eligible & covered, eligible, wrong


def runs_of(row):
    """bool [L] -> the maximal runs of True as (first, end) pairs, in order"""
    edges = np.diff(np.concatenate(([0], np.asarray(row, dtype=np.int8), [0])))
    return list(zip(np.nonzero(edges == 1)[0].tolist(), np.nonzero(edges == -1)[0].tolist()))


def span_corrupt_ref(ids_rows, mask, plan, *, seed, start_below, len_below, sentinel_first, sentinel_step=-1, n_sentinels=100,
                     target_eos_id=None, decoder_start_id=None, pad_id=0, ignore_index=-100, sides=T.SIDE_A | T.SIDE_B,
                     max_target_len=None, first_row=0):
    """ids_rows [n_rows, L], mask [n_rows, L], plan [n_rows, 8] ->
    (out_ids, out_mask, labels, input_lengths, target_lengths, decoder_input_ids or None, wrong)"""
    ids_rows, mask = np.asarray(ids_rows), np.asarray(mask)
    n_rows, L = ids_rows.shape
    L_tgt = L if max_target_len is None else max_target_len
    noise0, _eligible, wrong = noise_columns(mask, plan, seed=seed, start_below=start_below, len_below=len_below, sides=sides,
                                             first_row=first_row)
    out = np.full((n_rows, L), pad_id, dtype=ids_rows.dtype)
    out_mask = np.zeros((n_rows, L), dtype=np.uint8)
    labels = np.full((n_rows, L_tgt), ignore_index, dtype=ids_rows.dtype)
    dec = None if decoder_start_id is None else np.full((n_rows, L_tgt), pad_id, dtype=ids_rows.dtype)
    in_len, tgt_len = np.zeros(n_rows, dtype=np.int32), np.zeros(n_rows, dtype=np.int32)
    for r in range(n_rows):
        ids, real = ids_rows[r], mask[r] != 0
        row, target, at = [], [], 0
        for k, (first, end) in enumerate(runs_of(noise0[r])[:n_sentinels]):  # runs past the last sentinel stay text
            sentinel = sentinel_first + k * sentinel_step
            row += ids[at:first][real[at:first]].tolist() + [sentinel]
            target += [sentinel] + ids[first:end].tolist()
            at = end
        row += ids[at:][real[at:]].tolist()
        if target_eos_id is not None:
            target.append(target_eos_id)
        out[r, :len(row)] = row
        out_mask[r, :len(row)] = 1
        in_len[r], tgt_len[r] = len(row), len(target)
        target = target[:L_tgt]
        labels[r, :len(target)] = target
        if dec is not None:
            dec[r, 0] = decoder_start_id
            dec[r, 1:len(target) + 1] = target[:L_tgt - 1]
    return out, out_mask, labels, in_len, tgt_len, dec, wrong
