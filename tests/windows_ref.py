"""NumPy restatement of the window collation (include/hutoken_amd.h, WINDOWS), written from the
definitions: `windows` is a loop over documents and windows, `windows_vec` the same result from array operations (pinned
by the loop form in tests/test_windows_cpu.py) for batches the loop is too slow for.

  C = L - s ids fit a row (s: bos/eos tokens given), step = C - stride
  a document of n ids gives w(n) = 1 rows when n <= C, 1 + ceil((n - C) / step) otherwise
  window k holds the document's ids [k * step, min(k * step + C, n))
"""
import numpy as np


def ragged(docs):
    """list of lists -> (ids int32, offsets int64[n + 1])"""
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=offs[1:])
    ids = np.array([t for d in docs for t in d], dtype=np.int32)
    return ids, offs


def sizes(L, stride, bos_id, eos_id):
    s = (bos_id is not None) + (eos_id is not None)
    C = L - s
    assert L >= 1 and C >= 1 and 0 <= stride < C
    return s, C, C - stride


def window_count(n, C, step):
    return 1 if n <= C else 1 + -(-(n - C) // step)


def row_offsets(offs, L, stride=0, bos_id=None, eos_id=None):
    """int64[n_docs + 1]: the exclusive prefix sum of the documents' window counts."""
    _s, C, step = sizes(L, stride, bos_id, eos_id)
    out = np.zeros(len(offs), dtype=np.int64)
    for i in range(len(offs) - 1):
        out[i + 1] = out[i] + window_count(int(offs[i + 1] - offs[i]), C, step)
    return out


def windows(ids, offs, L, stride=0, bos_id=None, eos_id=None, pad_id=0, padding_side="right", dtype=np.int32):
    """-> (input_ids [n_rows, L] of dtype, attention_mask uint8 [n_rows, L], lengths int32 [n_rows],
    row_map int64 [n_rows, 2] = (document, index of the row's first id inside the document))"""
    _s, C, step = sizes(L, stride, bos_id, eos_id)
    rows, masks, lengths, row_map = [], [], [], []
    for d in range(len(offs) - 1):
        doc = [int(t) for t in ids[int(offs[d]):int(offs[d + 1])]]
        n = len(doc)
        for k in range(window_count(n, C, step)):
            seq = doc[k * step:min(k * step + C, n)]
            if bos_id is not None:
                seq = [bos_id] + seq
            if eos_id is not None:
                seq = seq + [eos_id]
            fill = [pad_id] * (L - len(seq))
            ones = [1] * len(seq)
            zeros = [0] * len(fill)
            rows.append(fill + seq if padding_side == "left" else seq + fill)
            masks.append(zeros + ones if padding_side == "left" else ones + zeros)
            lengths.append(len(seq))
            row_map.append((d, k * step))
    return (np.array(rows, dtype=dtype).reshape(len(rows), L), np.array(masks, dtype=np.uint8).reshape(len(rows), L),
            np.array(lengths, dtype=np.int32), np.array(row_map, dtype=np.int64).reshape(len(rows), 2))


def row_table(offs, L, stride=0, bos_id=None, eos_id=None):
    """Vectorised: (row_offsets int64[n_docs + 1], doc, start, n: int64[n_rows] each) -- every row's document, where its
    window starts in the document and how many of the document's ids it holds."""
    _s, C, step = sizes(L, stride, bos_id, eos_id)
    offs = np.asarray(offs, dtype=np.int64)
    lens = offs[1:] - offs[:-1]
    w = np.where(lens <= C, 1, 1 + (lens - C + step - 1) // step)
    ro = np.zeros(len(offs), dtype=np.int64)
    np.cumsum(w, out=ro[1:])
    doc = np.repeat(np.arange(len(lens), dtype=np.int64), w)
    start = (np.arange(int(ro[-1]), dtype=np.int64) - ro[doc]) * step
    n = np.minimum(lens[doc] - start, C)
    return ro, doc, start, n


def windows_vec(ids, offs, L, stride=0, bos_id=None, eos_id=None, pad_id=0, padding_side="right", dtype=np.int32):
    """windows() from array operations."""
    s, _C, _step = sizes(L, stride, bos_id, eos_id)
    has_bos = bos_id is not None
    _ro, doc, start, n = row_table(offs, L, stride, bos_id, eos_id)
    sl = n + s
    shift = L - sl if padding_side == "left" else np.zeros_like(sl)
    q = np.arange(L, dtype=np.int64)[None, :] - shift[:, None]
    valid = (q >= 0) & (q < sl[:, None])
    idx = np.asarray(offs, dtype=np.int64)[doc][:, None] + start[:, None] + q - has_bos
    src = np.concatenate([np.asarray(ids, dtype=np.int32), np.zeros(1, dtype=np.int32)])  # (never empty)
    out = np.where(valid, src[np.clip(idx, 0, len(src) - 1)], np.int32(pad_id)).astype(dtype)
    if has_bos:
        out[q == 0] = bos_id
    if eos_id is not None:
        out[q == sl[:, None] - 1] = eos_id
    return out, valid.astype(np.uint8), sl.astype(np.int32), np.stack([doc, start], axis=1).astype(np.int64)


def rows_bound(n_docs, n_ids, L, stride, s):
    """What hutk_windows_rows_bound returns."""
    return n_docs + n_ids // (L - s - stride)
