"""NumPy restatement of the pair collation (include/hutoken_amd.h, PAIRS), written from the
definitions: `pairs` and `pair_windows` are loops over pairs, windows and elements, `pairs_vec` and `pair_windows_vec`
the same results from array operations (pinned by the loop forms in tests/test_pairs_cpu.py) for batches the loops are
too slow for.

  a row is [bos] + A' + sep_ids + B' + [eos]; s = [bos] + len(sep_ids) + [eos]; R = L - s ids of room
  (ka, kb) = pair_lengths(na, nb, R, strategy); A' = A[:ka], B' = B[:kb]
  windows: the side that is not named keeps ko = min(no, R); the named one has C = R - ko per row, step = max(1, C - stride)
"""
import numpy as np

STRATEGIES = ("longest_first", "only_first", "only_second")


def ragged(docs, base=0, tail=0, junk=-77):
    """list of lists -> (ids int32, offsets int64[n + 1]) with `base` ids in front of the first document and `tail`
    behind the last that belong to none."""
    offs = np.full(len(docs) + 1, base, dtype=np.int64)
    if docs:
        offs[1:] += np.cumsum([len(d) for d in docs])
    ids = np.array([junk] * base + [t for d in docs for t in d] + [junk] * tail, dtype=np.int32)
    return ids, offs


def sizes(L, bos_id, sep_ids, eos_id):
    s = (bos_id is not None) + len(sep_ids) + (eos_id is not None)
    assert len(sep_ids) <= 4 and L - s >= 1
    return s, L - s


def pair_lengths(na, nb, R, strategy):
    if na + nb <= R:
        return na, nb
    if strategy == "only_first":
        kb = min(nb, R)
        return min(na, R - kb), kb
    if strategy == "only_second":
        ka = min(na, R)
        return ka, min(nb, R - ka)
    assert strategy == "longest_first"
    swap = na > nb
    n1, n2 = (nb, na) if swap else (na, nb)
    n2 = n1 if n1 > R else max(n1, R - n1)
    if n1 + n2 > R:
        n1 = R // 2
        n2 = n1 + R % 2
    return (n2, n1) if swap else (n1, n2)


def window_sizes(no, R, stride):
    """-> (ko, C, step) for a pair whose kept side has `no` ids"""
    ko = min(no, R)
    C = R - ko
    return ko, C, max(1, C - stride)


def window_count(n, no, R, stride):
    _ko, C, step = window_sizes(no, R, stride)
    return 1 if n <= C or C == 0 else 1 + -(-(n - C) // step)


def _row(A, B, bos_id, sep_ids, eos_id, pad_id, L, side):
    head = ([bos_id] if bos_id is not None else []) + A + list(sep_ids)
    back = B + ([eos_id] if eos_id is not None else [])
    seq, types = head + back, [0] * len(head) + [1] * len(back)
    fill = L - len(seq)
    assert fill >= 0
    if side == "left":
        return [pad_id] * fill + seq, [0] * fill + [1] * len(seq), [0] * fill + types, len(seq)
    return seq + [pad_id] * fill, [1] * len(seq) + [0] * fill, types + [0] * fill, len(seq)


def _docs(ids, offs, i):
    return [int(t) for t in ids[int(offs[i]):int(offs[i + 1])]]


def _arrays(rows, L, dtype, row_map=None):
    n = len(rows)
    out = (np.array([r[0] for r in rows], dtype=dtype).reshape(n, L), np.array([r[1] for r in rows], dtype=np.uint8).reshape(n, L),
           np.array([r[2] for r in rows], dtype=np.uint8).reshape(n, L), np.array([r[3] for r in rows], dtype=np.int32))
    return out if row_map is None else out + (np.array(row_map, dtype=np.int64).reshape(n, 2),)


def pairs(ids_a, offs_a, ids_b, offs_b, L, truncation="longest_first", bos_id=None, sep_ids=(), eos_id=None, pad_id=0,
          padding_side="right", dtype=np.int32):
    """-> (input_ids [n, L] of dtype, attention_mask uint8 [n, L], token_type_ids uint8 [n, L], lengths int32 [n])"""
    _s, R = sizes(L, bos_id, sep_ids, eos_id)
    rows = []
    for i in range(len(offs_a) - 1):
        A, B = _docs(ids_a, offs_a, i), _docs(ids_b, offs_b, i)
        ka, kb = pair_lengths(len(A), len(B), R, truncation)
        rows.append(_row(A[:ka], B[:kb], bos_id, sep_ids, eos_id, pad_id, L, padding_side))
    return _arrays(rows, L, dtype)


def pair_windows(ids_a, offs_a, ids_b, offs_b, L, stride=0, truncation="only_second", bos_id=None, sep_ids=(), eos_id=None,
                 pad_id=0, padding_side="right", dtype=np.int32):
    """-> pairs' four with one row per window, and row_map int64 [n_rows, 2] = (pair, where the window starts in the cut
    side)"""
    assert truncation in ("only_first", "only_second")
    _s, R = sizes(L, bos_id, sep_ids, eos_id)
    assert 0 <= stride < R
    rows, row_map = [], []
    for i in range(len(offs_a) - 1):
        A, B = _docs(ids_a, offs_a, i), _docs(ids_b, offs_b, i)
        cut, other = (B, A) if truncation == "only_second" else (A, B)
        ko, C, step = window_sizes(len(other), R, stride)
        for k in range(window_count(len(cut), len(other), R, stride)):
            piece = cut[k * step:min(k * step + C, len(cut))]
            a, b = (other[:ko], piece) if truncation == "only_second" else (piece, other[:ko])
            rows.append(_row(a, b, bos_id, sep_ids, eos_id, pad_id, L, padding_side))
            row_map.append((i, k * step))
    return _arrays(rows, L, dtype, row_map)


def row_offsets(offs_a, offs_b, L, stride=0, truncation="only_second", bos_id=None, sep_ids=(), eos_id=None):
    """int64[n + 1]: the exclusive prefix sum of the pairs' window counts, by the loop."""
    _s, R = sizes(L, bos_id, sep_ids, eos_id)
    out = np.zeros(len(offs_a), dtype=np.int64)
    for i in range(len(offs_a) - 1):
        na, nb = int(offs_a[i + 1] - offs_a[i]), int(offs_b[i + 1] - offs_b[i])
        n, no = (nb, na) if truncation == "only_second" else (na, nb)
        out[i + 1] = out[i] + window_count(n, no, R, stride)
    return out


def pair_lengths_vec(na, nb, R, strategy):
    na, nb = np.asarray(na, dtype=np.int64), np.asarray(nb, dtype=np.int64)
    if strategy == "only_first":
        kb = np.minimum(nb, R)
        ka = np.minimum(na, R - kb)
    elif strategy == "only_second":
        ka = np.minimum(na, R)
        kb = np.minimum(nb, R - ka)
    else:
        assert strategy == "longest_first"
        swap = na > nb
        n1, n2 = np.minimum(na, nb), np.maximum(na, nb)
        n2 = np.where(n1 > R, n1, np.maximum(n1, R - n1))
        over = n1 + n2 > R
        n1 = np.where(over, R // 2, n1)
        n2 = np.where(over, R // 2 + R % 2, n2)
        ka, kb = np.where(swap, n2, n1), np.where(swap, n1, n2)
    fits = na + nb <= R
    return np.where(fits, na, ka), np.where(fits, nb, kb)


def row_table(offs_a, offs_b, L, stride=0, truncation="only_second", bos_id=None, sep_ids=(), eos_id=None):
    """Vectorised: (row_offsets int64[n + 1], pair, start, ka, kb: int64[n_rows] each) -- every row's pair, where its
    window starts in the cut side and how many ids of A and of B it holds."""
    assert truncation in ("only_first", "only_second")
    _s, R = sizes(L, bos_id, sep_ids, eos_id)
    la = np.diff(np.asarray(offs_a, dtype=np.int64))
    lb = np.diff(np.asarray(offs_b, dtype=np.int64))
    n, no = (lb, la) if truncation == "only_second" else (la, lb)
    ko = np.minimum(no, R)
    C = R - ko
    step = np.maximum(1, C - stride)
    w = np.where((n <= C) | (C == 0), 1, 1 + (n - C + step - 1) // step)
    ro = np.zeros(len(la) + 1, dtype=np.int64)
    np.cumsum(w, out=ro[1:])
    pair = np.repeat(np.arange(len(la), dtype=np.int64), w)
    start = (np.arange(int(ro[-1]), dtype=np.int64) - ro[pair]) * step[pair]
    kn = np.minimum(n[pair] - start, C[pair])
    ka, kb = (ko[pair], kn) if truncation == "only_second" else (kn, ko[pair])
    return ro, pair, start, ka, kb


def expand(ids_a, offs_a, ids_b, offs_b, pair, start_a, start_b, ka, kb, L, bos_id, sep_ids, eos_id, pad_id, padding_side, dtype):
    """The rectangle of rows that hold A[start_a : start_a + ka] and B[start_b : start_b + kb] of `pair`."""
    s, _R = sizes(L, bos_id, sep_ids, eos_id)
    has_bos, n_sep = int(bos_id is not None), len(sep_ids)
    sl = ka + kb + s
    shift = L - sl if padding_side == "left" else np.zeros_like(sl)
    q = np.arange(L, dtype=np.int64)[None, :] - shift[:, None]
    valid = (q >= 0) & (q < sl[:, None])
    end_a = (has_bos + ka)[:, None]
    end_sep = end_a + n_sep
    end_b = end_sep + kb[:, None]
    in_a = valid & (q >= has_bos) & (q < end_a)
    in_b = valid & (q >= end_sep) & (q < end_b)
    src_a = np.concatenate([np.asarray(ids_a, dtype=np.int32), np.zeros(1, dtype=np.int32)])  # (never empty)
    src_b = np.concatenate([np.asarray(ids_b, dtype=np.int32), np.zeros(1, dtype=np.int32)])
    idx_a = np.asarray(offs_a, dtype=np.int64)[pair][:, None] + start_a[:, None] + q - has_bos
    idx_b = np.asarray(offs_b, dtype=np.int64)[pair][:, None] + start_b[:, None] + q - end_sep
    out = np.full(q.shape, pad_id, dtype=np.int32)
    out = np.where(in_a, src_a[np.clip(idx_a, 0, len(src_a) - 1)], out)
    out = np.where(in_b, src_b[np.clip(idx_b, 0, len(src_b) - 1)], out)
    if has_bos:
        out = np.where(valid & (q == 0), np.int32(bos_id), out)
    for u, t in enumerate(sep_ids):
        out = np.where(valid & (q == end_a + u), np.int32(t), out)
    if eos_id is not None:
        out = np.where(q == sl[:, None] - 1, np.int32(eos_id), out)
    types = valid & (q >= end_sep)
    return out.astype(dtype), valid.astype(np.uint8), types.astype(np.uint8), sl.astype(np.int32)


def pairs_vec(ids_a, offs_a, ids_b, offs_b, L, truncation="longest_first", bos_id=None, sep_ids=(), eos_id=None, pad_id=0,
              padding_side="right", dtype=np.int32):
    """pairs() from array operations."""
    _s, R = sizes(L, bos_id, sep_ids, eos_id)
    la, lb = np.diff(np.asarray(offs_a, dtype=np.int64)), np.diff(np.asarray(offs_b, dtype=np.int64))
    ka, kb = pair_lengths_vec(la, lb, R, truncation)
    pair = np.arange(len(la), dtype=np.int64)
    zero = np.zeros(len(la), dtype=np.int64)
    return expand(ids_a, offs_a, ids_b, offs_b, pair, zero, zero, ka, kb, L, bos_id, sep_ids, eos_id, pad_id, padding_side, dtype)


def pair_windows_vec(ids_a, offs_a, ids_b, offs_b, L, stride=0, truncation="only_second", bos_id=None, sep_ids=(),
                     eos_id=None, pad_id=0, padding_side="right", dtype=np.int32):
    """pair_windows() from array operations."""
    _ro, pair, start, ka, kb = row_table(offs_a, offs_b, L, stride, truncation, bos_id, sep_ids, eos_id)
    zero = np.zeros_like(start)
    sa, sb = (zero, start) if truncation == "only_second" else (start, zero)
    four = expand(ids_a, offs_a, ids_b, offs_b, pair, sa, sb, ka, kb, L, bos_id, sep_ids, eos_id, pad_id, padding_side, dtype)
    return four + (np.stack([pair, start], axis=1).astype(np.int64),)


def rows_bound(n_pairs, n_cut_ids):
    """What hutk_pair_rows_bound returns."""
    return n_pairs + n_cut_ids
