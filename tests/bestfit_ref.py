"""Plain restatement of best-fit packing (include/hutoken_amd.h, "BEST FIT"), written from the
rule, by the item-level definition: one item at a time into a sorted list of (room, bin).  tests/test_bestfit_cpu.py pins
it by hand.  Own code; nothing here touches the GPU or the package under test.

The rule.  L = seq_len; s = the number of bos/eos given.  Document i has n_i ids; its sequence is [bos] ids [eos],
m_i = n_i + s tokens.
  Whole rows: a sequence is cut every L tokens: w_i = m_i div L whole rows and, when m_i mod L > 0, one ITEM of length
  l_i = m_i mod L, the sequence's tail; m_i == 0 gives nothing.  Output rows 0 .. W - 1, W = sum of w_i, are the whole rows
  in document order, segment 1, positions 0 .. L - 1.
  Bins: the items are taken in the order (length descending, document number ascending).  Each goes into the open bin whose
  remaining room is the smallest that is still >= l, among bins of equal room the lowest-numbered one; if none fits a new
  bin opens with room L.  The item's column is L - room before it is placed, its segment id the number of items already
  in the bin plus 1, its positions 0 .. l - 1.  Bin b is output row W + b.  Behind a bin's last item: pad_id, position
  0, segment 0.  n_rows = W + B."""
import bisect

import numpy as np


def plan(offsets, L, s):
    """-> (doc_map int64 [n_docs, 4] = (whole_row, n_whole, row, col), segment of every item (0: none), room left in
    every bin, W)"""
    offsets = [int(o) for o in offsets]
    n_docs = len(offsets) - 1
    m = [offsets[i + 1] - offsets[i] + s for i in range(n_docs)]
    doc_map = np.full((n_docs, 4), -1, dtype=np.int64)
    W = 0
    for i in range(n_docs):
        doc_map[i, 1] = m[i] // L
        if m[i] // L:
            doc_map[i, 0] = W
            W += m[i] // L
    items = sorted((i for i in range(n_docs) if m[i] % L), key=lambda i: (-(m[i] % L), i))
    open_bins = []  # (room, bin), sorted
    rooms, count = [], []
    seg = np.zeros(n_docs, dtype=np.int64)
    for i in items:
        l = m[i] % L
        at = bisect.bisect_left(open_bins, (l, -1))  # the smallest room that is still >= l, its lowest bin
        if at < len(open_bins):
            room, b = open_bins.pop(at)
        else:
            room, b = L, len(rooms)
            rooms.append(L)
            count.append(0)
        doc_map[i, 2], doc_map[i, 3] = W + b, L - room
        count[b] += 1
        seg[i] = count[b]
        rooms[b] = room - l
        if room - l > 0:
            bisect.insort(open_bins, (room - l, b))
    return doc_map, seg, rooms, W


def pack(ids, offsets, L, bos_id=None, eos_id=None, pad_id=0, dtype=np.int32, rows_cap=None):
    """-> dict(input_ids, position_ids, segment_ids, lengths, source, doc_map, info) as the rule gives them; rows_cap:
    the rows of the arrays (None: n_rows), those behind n_rows all padding"""
    ids = np.asarray(ids, dtype=np.int32)
    s = (bos_id is not None) + (eos_id is not None)
    doc_map, seg, rooms, W = plan(offsets, L, s)
    n_rows = W + len(rooms)
    R = n_rows if rows_cap is None else rows_cap
    assert R >= n_rows
    out = {"input_ids": np.full((R, L), pad_id, dtype=dtype), "position_ids": np.zeros((R, L), dtype=np.int32),
           "segment_ids": np.zeros((R, L), dtype=np.int32), "lengths": np.zeros(R, dtype=np.int32),
           "source": np.full((R, L), -1, dtype=np.int64), "doc_map": doc_map, "info": (n_rows, W)}
    flat = {k: out[k].reshape(-1) for k in ("input_ids", "position_ids", "segment_ids", "source")}
    for i in range(len(offsets) - 1):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        head, tail = ([bos_id] if bos_id is not None else []), ([eos_id] if eos_id is not None else [])
        tok = np.concatenate([np.array(head, dtype=np.int64), ids[o0:o1].astype(np.int64), np.array(tail, dtype=np.int64)])
        src = np.concatenate([np.full(len(head), -1, dtype=np.int64), np.arange(o0, o1, dtype=np.int64),
                              np.full(len(tail), -1, dtype=np.int64)])
        first, n_whole, row, col = (int(x) for x in doc_map[i])
        pieces = [(first * L, 0, n_whole * L, None)] if n_whole else []
        if row >= 0:
            pieces.append((row * L + col, n_whole * L, len(tok), int(seg[i])))
        for at, t0, t1, sg in pieces:
            n = t1 - t0
            flat["input_ids"][at:at + n] = tok[t0:t1]
            flat["source"][at:at + n] = src[t0:t1]
            flat["segment_ids"][at:at + n] = 1 if sg is None else sg
            flat["position_ids"][at:at + n] = np.arange(n) % L
    out["lengths"][:W] = L
    for b, room in enumerate(rooms):
        out["lengths"][W + b] = L - room
    return out


def rows_bound(n_docs, n_ids, L, s):
    """the bound of hutk_bestfit_rows_bound, restated: min(2 T div L + 1, T div L + n_docs), 0 without documents"""
    T = n_ids + s * n_docs
    return 0 if n_docs == 0 else min(2 * T // L + 1, T // L + n_docs)
