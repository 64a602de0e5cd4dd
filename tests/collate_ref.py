"""NumPy restatement of the collation semantics (include/hutoken_amd.h, "collation").

Two forms of each layout: a plain loop written from the definitions (the contract; tests/test_collate_cpu.py pins it with
hand-written expectations) and a vectorised one for the full-size GPU tests, which the loop form pins on random inputs.
Own code; nothing here touches the GPU or the package under test."""
import bisect

import numpy as np


def sequence(doc, bos_id, eos_id):
    return ([bos_id] if bos_id is not None else []) + [int(x) for x in doc] + ([eos_id] if eos_id is not None else [])


def docs_of(ids, offsets):
    return [ids[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def ragged(docs):
    """list of int lists -> (ids int32, offsets int64[n + 1])"""
    offsets = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=offsets[1:])
    ids = np.fromiter((x for d in docs for x in d), dtype=np.int64, count=int(offsets[-1])).astype(np.int32)
    return ids, offsets


# ---- padded -------------------------------------------------------------------------------------------------------
def padded(ids, offsets, max_length, bos_id=None, eos_id=None, pad_id=0, truncation="right", padding_side="right",
           dtype=np.int32):
    """-> (input_ids [n, L], attention_mask uint8 [n, L], lengths int32 [n])"""
    L = int(max_length)
    s = (bos_id is not None) + (eos_id is not None)
    assert L >= max(1, s)
    n = len(offsets) - 1
    out = np.full((n, L), pad_id, dtype=dtype)
    mask = np.zeros((n, L), dtype=np.uint8)
    lengths = np.zeros(n, dtype=np.int32)
    for i, doc in enumerate(docs_of(ids, offsets)):
        if len(doc) + s > L:
            doc = doc[:L - s] if truncation == "right" else doc[len(doc) - (L - s):]
        seq = sequence(doc, bos_id, eos_id)
        lengths[i] = len(seq)
        at = 0 if padding_side == "right" else L - len(seq)
        out[i, at:at + len(seq)] = seq
        mask[i, at:at + len(seq)] = 1
    return out, mask, lengths


def padded_vec(ids, offsets, max_length, bos_id=None, eos_id=None, pad_id=0, truncation="right",
               padding_side="right", dtype=np.int32, rows=None, block=65536):
    """The same without a Python loop over documents; `rows` = (first, last) restricts the output to those rows."""
    L = int(max_length)
    has_bos, has_eos = bos_id is not None, eos_id is not None
    s = has_bos + has_eos
    offsets = np.asarray(offsets, dtype=np.int64)
    a, b = (0, len(offsets) - 1) if rows is None else rows
    out = np.empty((b - a, L), dtype=dtype)
    mask = np.empty((b - a, L), dtype=np.uint8)
    lengths = np.empty(b - a, dtype=np.int32)
    col = np.arange(L, dtype=np.int64)[None, :]
    safe = ids if len(ids) else np.zeros(1, dtype=np.int32)
    for r0 in range(a, b, block):
        r1 = min(r0 + block, b)
        o0, o1 = offsets[r0:r1], offsets[r0 + 1:r1 + 1]
        n = np.minimum(o1 - o0, L - s)
        sl = n + s
        src = o0 if truncation == "right" else o1 - n
        shift = np.zeros_like(sl) if padding_side == "right" else L - sl
        q = col - shift[:, None]
        valid = (q >= 0) & (q < sl[:, None])
        idx = np.clip(src[:, None] + q - has_bos, 0, len(safe) - 1)
        v = np.where(valid, safe[idx], pad_id)
        if has_eos:
            v = np.where(valid & (q == sl[:, None] - 1), eos_id, v)
        if has_bos:
            v = np.where(valid & (q == 0), bos_id, v)
        out[r0 - a:r1 - a] = v
        mask[r0 - a:r1 - a] = valid
        lengths[r0 - a:r1 - a] = sl
    return out, mask, lengths


# ---- packed -------------------------------------------------------------------------------------------------------
def _empty_rows(L, dtype):
    return {"input_ids": np.zeros((0, L), dtype=dtype), "position_ids": np.zeros((0, L), dtype=np.int32),
            "segment_ids": np.zeros((0, L), dtype=np.int32)}


def cat_rows(parts, L, dtype=np.int32):
    parts = [p for p in parts if len(p["input_ids"])]
    if not parts:
        return _empty_rows(L, dtype)
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def rows_equal(a, b):
    return all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k])
               for k in ("input_ids", "position_ids", "segment_ids"))


class Packer:
    """The stateful packer, from the definitions: the stream S since the last flush, the start b_j of every non-empty
    sequence, and for stream index p in row k = p // L:
        input_ids = S[p], position_ids = p - max(b_j, k L) for the sequence j that holds p,
        segment_ids = 1 + #{ j' : k L < b_j' <= p }."""

    def __init__(self, seq_len, bos_id=None, eos_id=None, pad_id=0, dtype=np.int32):
        self.L, self.bos_id, self.eos_id, self.pad_id, self.dtype = int(seq_len), bos_id, eos_id, pad_id, dtype
        self.S, self.starts, self.done = [], [], 0  # done: rows already returned

    @property
    def pending(self):
        return len(self.S) - self.done * self.L

    def _row(self, k, upto):
        L = self.L
        ids = np.full(L, self.pad_id, dtype=self.dtype)
        pos = np.zeros(L, dtype=np.int32)
        seg = np.zeros(L, dtype=np.int32)
        for p in range(k * L, upto):
            j = bisect.bisect_right(self.starts, p) - 1
            ids[p - k * L] = self.S[p]
            pos[p - k * L] = p - max(self.starts[j], k * L)
            seg[p - k * L] = 1 + bisect.bisect_right(self.starts, p) - bisect.bisect_right(self.starts, k * L)
        return ids, pos, seg

    def _stack(self, rows):
        if not rows:
            return _empty_rows(self.L, self.dtype)
        return {"input_ids": np.stack([r[0] for r in rows]), "position_ids": np.stack([r[1] for r in rows]),
                "segment_ids": np.stack([r[2] for r in rows])}

    def add(self, ids, offsets):
        for doc in docs_of(ids, offsets):
            seq = sequence(doc, self.bos_id, self.eos_id)
            if seq:
                self.starts.append(len(self.S))
                self.S.extend(seq)
        rows = []
        while (self.done + 1) * self.L <= len(self.S):
            rows.append(self._row(self.done, (self.done + 1) * self.L))
            self.done += 1
        return self._stack(rows)

    def flush(self):
        rows = [self._row(self.done, len(self.S))] if self.pending else []
        self.S, self.starts, self.done = [], [], 0
        return self._stack(rows)


def packed_vec(ids, offsets, seq_len, bos_id=None, eos_id=None, pad_id=0, dtype=np.int32):
    """All documents in one add, then flush, without a Python loop: -> (complete rows, flushed rows (0 or 1))."""
    L = int(seq_len)
    has_bos, has_eos = bos_id is not None, eos_id is not None
    s = has_bos + has_eos
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets) + s
    keep = lens > 0
    lens, o0 = lens[keep], offsets[:-1][keep]
    b = np.zeros(len(lens), dtype=np.int64)
    if len(lens):
        np.cumsum(lens[:-1], out=b[1:])
    T = int(lens.sum())
    n_rows = -(-T // L)
    j = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    p = np.arange(T, dtype=np.int64)
    q = p - b[j]
    safe = ids if len(ids) else np.zeros(1, dtype=np.int32)
    S = safe[np.clip(o0[j] + q - has_bos, 0, len(safe) - 1)].astype(dtype)
    if has_eos:
        S[q == lens[j] - 1] = eos_id
    if has_bos:
        S[q == 0] = bos_id
    row_start = p // L * L
    pos = (p - np.maximum(b[j], row_start)).astype(np.int32)
    f = np.zeros(T, dtype=np.int32)
    f[b] = 1
    f[::L] = 0  # a start AT the row's start is not counted (k L < b)
    c = np.cumsum(f, dtype=np.int64)
    seg = (1 + c - c[row_start]).astype(np.int32) if T else np.zeros(0, dtype=np.int32)
    del j, p, q, f, c, row_start
    full = {"input_ids": np.full(n_rows * L, pad_id, dtype=dtype), "position_ids": np.zeros(n_rows * L, dtype=np.int32),
            "segment_ids": np.zeros(n_rows * L, dtype=np.int32)}
    full["input_ids"][:T] = S
    full["position_ids"][:T] = pos
    full["segment_ids"][:T] = seg
    full = {k: v.reshape(n_rows, L) for k, v in full.items()}
    whole = T // L
    return {k: v[:whole] for k, v in full.items()}, {k: v[whole:] for k, v in full.items()}
