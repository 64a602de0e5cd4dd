"""Fill-in-the-middle in plain numpy and Python: the definitions that k_fim_cut, k_fim_plan and k_fim_render of
csrc/hutk_collate.hip are tested against (include/hutoken_amd.h states the rule in full).

THE RULE, restated.  Sentinels pre, suf, mid are required, end is optional and stands behind the middle of transformed
documents only; E = 1 with an end.  Kinds: 0 plain, 1 PSM, 2 SPM.  Parts: 0 plain, 1 prefix, 2 middle, 3 suffix,
4 sentinel; loss_parts is a mask of 1 << part, and LOSS_END = 1 << 5 in it names the end sentinel alone.

Document number d = first_doc + i draws (u0, u1, u2, u3) = targets_ref.draw(seed, d, 0, DRAW_FIM = 4).  With len the
document's length it is transformed iff u0 < fim_below and 1 <= len < 2**31, SPM iff transformed and u1 < spm_below,
else PSM; a = (u2 * (len + 1)) >> 32, b = (u3 * (len + 1)) >> 32, lo = min(a, b), hi = max(a, b).  A plain document has
lo = hi = len.  The thresholds are ints in 0 .. 2**32.

Token level: len = n, the id count.  prefix = x[0:lo], middle = x[lo:hi], suffix = x[hi:n].
    plain  x
    PSM    pre prefix suf suffix mid middle [end]
    SPM    pre suf suffix mid prefix middle [end]
A transformed document has n + 3 + E outputs; out_offsets is the exclusive scan.  Per output: the id, the label (the id
where loss_parts has the part, else ignore_index), the part, the source (the index into ids, -1 on sentinels).

Character level: len = the byte count; each cut moves back to a UTF-8 character start: while 0 < pos < len, bytes[pos] is
in 0x80 .. 0xBF and fewer than three steps were taken, pos -= 1.  piece_offsets[3i .. 3i + 2] = start, start + lo,
start + hi, piece_offsets[3 n_docs] = the end of the text; a plain document is (whole, empty, empty).  After ONE encode
over the 3 n_docs pieces, lo / hi / n of document i are read from the ids' offsets [3i .. 3i + 3] and the kind from
kinds; nothing is drawn."""
import numpy as np

import targets_ref as T

DRAW_FIM = 4
PLAIN, PSM, SPM = 0, 1, 2
PART_PLAIN, PART_PREFIX, PART_MIDDLE, PART_SUFFIX, PART_SENTINEL = 0, 1, 2, 3, 4
LOSS_END = 32
LOSS_ALL = 31
LOSS_MIDDLE = (1 << PART_MIDDLE) | (1 << PART_PLAIN) | LOSS_END
E_ARG, E_CAPACITY = 4, 7


def decide(seed, doc, length, fim_below, spm_below):
    """arrays (or ints) -> (kind, lo, hi) as int64 arrays"""
    doc, length = np.broadcast_arrays(np.asarray(doc, dtype=np.uint64), np.asarray(length, dtype=np.int64))
    u0, u1, u2, u3 = T.draw(seed, doc, 0, DRAW_FIM)
    ok = (length >= 1) & (length < 2**31)
    m = np.where(ok, length + 1, 1).astype(np.uint64)  # (u * m < 2**64 where it counts)
    a = ((u2 * m) >> np.uint64(32)).astype(np.int64)
    b = ((u3 * m) >> np.uint64(32)).astype(np.int64)
    transformed = (u0 < np.uint64(fim_below)) & ok
    kind = np.where(transformed, np.where(u1 < np.uint64(spm_below), SPM, PSM), PLAIN).astype(np.int64)
    lo = np.where(transformed, np.minimum(a, b), length)
    hi = np.where(transformed, np.maximum(a, b), length)
    return kind, lo, hi


def rendered_length(n, kind, E):
    return n if kind == PLAIN else n + 3 + E


def layout(n, lo, hi, kind, E):
    """The rendered document as a list of (part, v): v the index inside the document, or the sentinel's number
    (0 pre, 1 suf, 2 mid, 3 end)."""
    pre, mid, suf = [(PART_PREFIX, k) for k in range(lo)], [(PART_MIDDLE, k) for k in range(lo, hi)], [(PART_SUFFIX, k) for k in range(hi, n)]
    S = PART_SENTINEL
    if kind == PLAIN:
        return [(PART_PLAIN, k) for k in range(n)]
    end = [(S, 3)] if E else []
    if kind == PSM:
        return [(S, 0)] + pre + [(S, 1)] + suf + [(S, 2)] + mid + end
    return [(S, 0), (S, 1)] + suf + [(S, 2)] + pre + mid + end


def char_start(doc_bytes, pos):
    steps = 0
    while 0 < pos < len(doc_bytes) and 0x80 <= doc_bytes[pos] <= 0xBF and steps < 3:
        pos -= 1
        steps += 1
    return pos


def cut_text(data, offsets, *, seed, fim_below, spm_below, first_doc=0):
    """packed text -> (piece_offsets int64[3 n + 1], kinds int32[n])"""
    data, offsets = bytes(data), [int(o) for o in offsets]
    n = len(offsets) - 1
    lens = np.array([offsets[i + 1] - offsets[i] for i in range(n)], dtype=np.int64)
    kind, lo, hi = decide(seed, first_doc + np.arange(n, dtype=np.int64), lens, fim_below, spm_below) if n else ((), (), ())
    pieces = np.zeros(3 * n + 1, dtype=np.int64)
    for i in range(n):
        s, doc = offsets[i], data[offsets[i]:offsets[i + 1]]
        l, h = int(lo[i]), int(hi[i])
        if kind[i] != PLAIN:
            l, h = char_start(doc, l), char_start(doc, h)
        pieces[3 * i:3 * i + 3] = (s, s + l, s + h)
    pieces[3 * n] = offsets[n]
    return pieces, np.asarray(kind, dtype=np.int32).reshape(n)


def plan_tokens(offsets, *, seed, fim_below, spm_below, first_doc=0):
    """-> (plan int64[n, 4] = (src0, n, lo, hi), kinds int32[n])"""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    lens = offsets[1:] - offsets[:-1]
    kind, lo, hi = decide(seed, first_doc + np.arange(n, dtype=np.int64), lens, fim_below, spm_below)
    return np.stack([offsets[:-1], lens, lo, hi], axis=1).astype(np.int64).reshape(n, 4), kind.astype(np.int32)


def plan_pieces(piece_id_offsets):
    """the ids' offsets of the 3 n pieces -> plan int64[n, 4]"""
    o = np.asarray(piece_id_offsets, dtype=np.int64)
    a, b, c, e = o[0:-1:3], o[1::3], o[2::3], o[3::3]
    return np.stack([a, e - a, b - a, c - a], axis=1).astype(np.int64)


def render(ids, plan, kinds, *, pre, suf, mid, end=None, loss_parts=LOSS_ALL, ignore_index=-100):
    """-> dict(out_ids, out_offsets, labels, parts, source): every output element by element from layout()"""
    ids = np.asarray(ids, dtype=np.int64)
    E = 0 if end is None else 1
    sent = (pre, suf, mid, end)
    out, lab, par, src, oo = [], [], [], [], [0]
    for (src0, n, lo, hi), kind in zip(np.asarray(plan).reshape(-1, 4).tolist(), np.asarray(kinds).tolist()):
        for part, v in layout(n, lo, hi, kind, E):
            tok = sent[v] if part == PART_SENTINEL else int(ids[src0 + v])
            loss = (loss_parts >> part) & 1 or (part == PART_SENTINEL and v == 3 and loss_parts & LOSS_END)
            out.append(tok)
            lab.append(tok if loss else ignore_index)
            par.append(part)
            src.append(-1 if part == PART_SENTINEL else src0 + v)
        oo.append(len(out))
    return {"out_ids": np.array(out, dtype=np.int32), "out_offsets": np.array(oo, dtype=np.int64),
            "labels": np.array(lab, dtype=np.int32), "parts": np.array(par, dtype=np.int32),
            "source": np.array(src, dtype=np.int64)}


def fim_tokens(ids, offsets, *, seed, fim_below, spm_below, first_doc=0, **kw):
    plan, kinds = plan_tokens(offsets, seed=seed, fim_below=fim_below, spm_below=spm_below, first_doc=first_doc)
    r = render(ids, plan, kinds, **kw)
    r["plan"], r["kinds"] = plan, kinds
    return r
