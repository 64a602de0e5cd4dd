"""Row-aligned features in plain Python: the definitions that the GPU kernels of csrc/hutk_collate.hip (row plans, the
gather, answer positions) and csrc/hutk_features.hip (word ids) are tested against.

A row plan is (item, start, src_a, ka, col_a, src_b, kb, col_b): columns col_a .. col_a + ka - 1 of the row hold
ids_a[src_a ..], columns col_b .. col_b + kb - 1 hold ids_b[src_b ..], every other column is bos, a separator, eos or
padding.  The plans of the four layouts are restated here on their own, by loops over documents and windows;
tests/test_features_cpu.py holds them against collate_ref / windows_ref / pairs_ref by rebuilding input_ids from
plan + ids + template (rebuild below)."""
import bisect

import numpy as np


def _place(L, side, has_bos, n_sep, s, ka, kb):
    """-> (col_a, col_b) of a row that keeps ka and kb ids"""
    shift = L - (ka + kb + s) if side == "left" else 0
    col_a = shift + has_bos
    return col_a, col_a + ka + n_sep


def padded_plan(offs, L, bos_id=None, eos_id=None, truncation="right", padding_side="right"):
    has_bos = int(bos_id is not None)
    s = has_bos + (eos_id is not None)
    rows = []
    for i in range(len(offs) - 1):
        n = int(offs[i + 1] - offs[i])
        ka = min(n, L - s)
        start = n - ka if truncation == "left" else 0
        col_a, col_b = _place(L, padding_side, has_bos, 0, s, ka, 0)
        rows.append((i, start, int(offs[i]) + start, ka, col_a, 0, 0, col_b))
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def windows_plan(offs, L, stride=0, bos_id=None, eos_id=None, padding_side="right"):
    has_bos = int(bos_id is not None)
    s = has_bos + (eos_id is not None)
    C = L - s
    step = C - stride
    assert C >= 1 and 0 <= stride < C
    rows = []
    for i in range(len(offs) - 1):
        n = int(offs[i + 1] - offs[i])
        start = 0
        while True:
            ka = min(C, n - start)
            col_a, col_b = _place(L, padding_side, has_bos, 0, s, ka, 0)
            rows.append((i, start, int(offs[i]) + start, ka, col_a, 0, 0, col_b))
            if start + C >= n:  # this window reaches the document's end
                break
            start += step
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def kept(na, nb, R, strategy):
    """(ka, kb) by taking one id away at a time, as the strategies are described"""
    ka, kb = na, nb
    while ka + kb > R:
        if strategy == "only_first":
            from_a = ka > 0 and (kb <= R)  # A gives way until it is empty; B only when it alone exceeds the room
        elif strategy == "only_second":
            from_a = not (kb > 0 and ka <= R)
        else:  # the longer side; of two equal ones the one that was shorter at first (B when they were equal: A gives way)
            from_a = ka > kb or (ka == kb and na <= nb)
        if from_a:
            ka -= 1
        else:
            kb -= 1
    return ka, kb


def pairs_plan(offs_a, offs_b, L, truncation="longest_first", bos_id=None, sep_ids=(), eos_id=None, padding_side="right"):
    has_bos, n_sep = int(bos_id is not None), len(sep_ids)
    s = has_bos + n_sep + (eos_id is not None)
    rows = []
    for i in range(len(offs_a) - 1):
        ka, kb = kept(int(offs_a[i + 1] - offs_a[i]), int(offs_b[i + 1] - offs_b[i]), L - s, truncation)
        col_a, col_b = _place(L, padding_side, has_bos, n_sep, s, ka, kb)
        rows.append((i, 0, int(offs_a[i]), ka, col_a, int(offs_b[i]), kb, col_b))
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def pair_windows_plan(offs_a, offs_b, L, stride=0, truncation="only_second", bos_id=None, sep_ids=(), eos_id=None,
                      padding_side="right"):
    assert truncation in ("only_first", "only_second")
    has_bos, n_sep = int(bos_id is not None), len(sep_ids)
    s = has_bos + n_sep + (eos_id is not None)
    R = L - s
    rows = []
    for i in range(len(offs_a) - 1):
        na, nb = int(offs_a[i + 1] - offs_a[i]), int(offs_b[i + 1] - offs_b[i])
        n, no = (nb, na) if truncation == "only_second" else (na, nb)
        ko = min(no, R)
        C = R - ko
        step = max(1, C - stride)
        start = 0
        while True:
            kn = max(0, min(C, n - start))
            ka, kb = (ko, kn) if truncation == "only_second" else (kn, ko)
            sa, sb = (0, start) if truncation == "only_second" else (start, 0)
            col_a, col_b = _place(L, padding_side, has_bos, n_sep, s, ka, kb)
            rows.append((i, start, int(offs_a[i]) + sa, ka, col_a, int(offs_b[i]) + sb, kb, col_b))
            if C == 0 or start + C >= n:
                break
            start += step
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def gather(plan, L, values_a, values_b=None, fill=0):
    """values [n] or [n, 2] -> [n_rows, L] or [n_rows, L, 2]: the token's value on the A and B columns, fill elsewhere"""
    values_a = np.asarray(values_a)
    values_b = values_a if values_b is None else np.asarray(values_b)
    out = np.empty((len(plan), L) + values_a.shape[1:], dtype=values_a.dtype)
    out[...] = np.asarray(fill, dtype=values_a.dtype)
    for r, (_item, _start, src_a, ka, col_a, src_b, kb, col_b) in enumerate(np.asarray(plan).tolist()):
        out[r, col_a:col_a + ka] = values_a[src_a:src_a + ka]
        out[r, col_b:col_b + kb] = values_b[src_b:src_b + kb]
    return out


def rebuild(plan, L, ids_a, ids_b=None, bos_id=None, sep_ids=(), eos_id=None, pad_id=0, dtype=np.int32):
    """input_ids from plan + ids + template: the ids by the gather, the template's tokens around them"""
    out = gather(plan, L, np.asarray(ids_a).astype(dtype), None if ids_b is None else np.asarray(ids_b).astype(dtype), pad_id)
    for r, (_item, _start, _sa, ka, col_a, _sb, kb, col_b) in enumerate(np.asarray(plan).tolist()):
        if bos_id is not None:
            out[r, col_a - 1] = bos_id
        for u, t in enumerate(sep_ids):
            out[r, col_a + ka + u] = t
        if eos_id is not None:
            out[r, col_b + kb] = eos_id
    return out


def word_ids(doc, byte_spans, starts):
    """The word each token starts in -- starts: the ascending byte offsets of the document's word starts
    (presplit_ref.word_starts) -- and whether some non-empty span holds a word start strictly inside it.
    -> (list of int, mismatch)"""
    out, mismatch = [], False
    for a, b in byte_spans:
        a, b = int(a), int(b)
        out.append(bisect.bisect_right(starts, a) - 1)
        if b > a and bisect.bisect_left(starts, b) > bisect.bisect_right(starts, a):
            mismatch = True
    return out, mismatch


def answer(spans, col, s, e):
    """The closed form: spans (a_j, b_j) of a row's tokens of one side, non-decreasing; col the column of the first.
    -> (start column, end column), (-1, -1) when the row does not hold the whole answer or there is none."""
    k = len(spans)
    if s >= e or k == 0 or spans[0][0] > s or spans[k - 1][1] < e:
        return -1, -1
    js = max(j for j in range(k) if spans[j][0] <= s)
    je = min(j for j in range(k) if spans[j][1] >= e)
    return col + js, col + je


def answers(plan, side, spans, ans):
    """answer() over a plan: side "a" or "b", spans [n, 2] indexed like that side's ids, ans [n_items, 2] -> int32 [n_rows, 2]"""
    out = np.empty((len(plan), 2), dtype=np.int32)
    for r, row in enumerate(np.asarray(plan).tolist()):
        src, k, col = row[5:8] if side == "b" else row[2:5]
        s, e = (int(x) for x in ans[row[0]])
        out[r] = answer([tuple(int(x) for x in sp) for sp in spans[src:src + k]], col, s, e)
    return out
