"""Special tokens, restated from the contract of include/hutoken_amd.h in plain Python (own code).

split() is the left-to-right scan of the contract; encode() cuts every document at the matches, sends the text pieces
through the CPU oracle as documents of their own and puts the special ids between them.  tests/test_specials_cpu.py
pins split() by hand and against Python's `re`; tests/test_gpu_specials.py compares the GPU with encode()."""
import numpy as np


def split(doc, specials):
    """doc: bytes of ONE document; specials: {bytes: id}.  -> [(start, end, id)]: leftmost first, then longest, never
    overlapping, every match inside the document."""
    by_len = sorted(specials, key=len, reverse=True)
    out, cur, n = [], 0, len(doc)
    while cur < n:
        for s in by_len:  # the longest that matches at the cursor and ends inside the document
            if doc.startswith(s, cur):
                out.append((cur, cur + len(s), specials[s]))
                cur += len(s)
                break
        else:
            cur += 1
    return out


def pieces(doc, specials):
    """-> [bytes | int]: text pieces (possibly empty) and special ids in turn, text first and last."""
    out, cur = [], 0
    for a, b, i in split(doc, specials):
        out.append(doc[cur:a])
        out.append(i)
        cur = b
    out.append(doc[cur:])
    return out


def encode(oracle, data, offsets, specials):
    """The contract's encoding of a packed batch -> (ids int32, out_offsets int64[n + 1], status int32[n], matches)."""
    raw = bytes(np.asarray(data, dtype=np.uint8).tobytes())
    n = len(offsets) - 1
    plan, texts = [], []  # per document: [("t", index into texts) | ("s", id)]
    matches = 0
    for d in range(n):
        row = []
        for p in pieces(raw[int(offsets[d]):int(offsets[d + 1])], specials):
            if isinstance(p, bytes):
                row.append(("t", len(texts)))
                texts.append(p)
            else:
                row.append(("s", p))
                matches += 1
        plan.append(row)
    t_offs = np.zeros(len(texts) + 1, dtype=np.int64)
    if texts:
        np.cumsum([len(t) for t in texts], out=t_offs[1:])
    t_data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    if texts:
        t_ids, t_oo, t_st = oracle.encode_packed(t_data, t_offs)
    else:
        t_ids, t_oo, t_st = np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32)
    parts, oo, st = [], np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    total = 0
    for d, row in enumerate(plan):
        for kind, v in row:
            if kind == "t":
                seg = t_ids[int(t_oo[v]):int(t_oo[v + 1])]
                parts.append(np.asarray(seg, dtype=np.int32))
                total += len(seg)
                st[d] = max(st[d], int(t_st[v]))
            else:
                parts.append(np.array([v], dtype=np.int32))
                total += 1
        oo[d + 1] = total
    ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    return ids.astype(np.int32, copy=False), oo, st, matches
