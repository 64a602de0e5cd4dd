"""Row passes, packed rows, the chat render and fill-in-the-middle on batches whose flat positions pass a boundary B:
what tests/test_gpu_wide_rows.py runs on the GPU (B = 2^31 and 2^32 elements) and tests/test_wide_rows_cpu.py holds to
its claims without one (B = 2^16 and 2^17).  The pattern is that of tests/wide_cases.py; every builder takes B.

Rows.  rows_shape(B, L) gives n_rows = B // L + 64 rows of L columns.  The band [B // L - 64, B // L + 64) holds rows on
both sides of flat element B and the last 64 rows lie past it -- wholly, but for the first of them when L does not
divide B: with L = 2047 the boundary falls inside that row.
padded_docs() draws the documents of such a batch (lengths 0 .. 40, about 50 of 5000 that get truncated, a truncated and
an empty one on either side of the boundary inside the band).

    deterministic passes   torch_lm_labels, torch_gather, torch_packed_labels: plain torch expressions over a slice of
                           rows, on whatever device their inputs are on; assert_rect() compares the WHOLE rectangle with
                           them slice by slice.  The CPU test holds them against targets_ref.labels_ref,
                           features_ref.gather and packed_ref.labels.
    random passes          mlm_band() and span_band() cut rows [a, b) out and call targets_ref.mlm_ref and
                           span_ref.span_corrupt_ref with first_row = a; mlm_invariants() and span_invariants() check
                           every element and every row of the whole rectangle in slices (no temporary above 1 GiB).

Packed stream.  packed_stream() draws documents whose every `sync_every`-th is lengthened so that the stream up to it is a
multiple of L: a document starts at a row's first element there (a sync point), and packed_ref.Packer fed only the
documents between two sync points gives the rows between them exactly.  Two channels, 4-byte and 16-byte records whose
values are a function of the flat id index, so that a misplaced record identifies itself.

Chat and fill-in-the-middle (pieces level).  One block of conversations (documents) whose rendered length is odd
(wide_cases.choose_length), with a conversation end, a bos, a turn start and an empty turn laid across p = B mod n_out;
the batch is R copies and equals the block's render in every copy (assert_copies, assert_copy_offsets).
Fill-in-the-middle at token level draws by the document's number, so copies differ: fim_band() runs fim_ref on the
documents around a place, fim_totals() checks two values over everything.

Every checker names the row or copy, the flat position and the side of the boundary.  Nothing here touches the package
under test."""
import math
import random

import numpy as np

import chat_ref
import fim_ref
import packed_ref
import span_ref
import targets_ref
import wide_cases as W

IGN = -100
BOS, EOS, PAD = 1, 2, 0
ID_LO, ID_HI = 1000, 2000       # the ids of the rows
VOCAB, MASK_ID = 1000, 5000     # random replacements lie below the ids, the mask id above: the three kinds are disjoint
SENT_FIRST, N_SENT = 60000, 100  # span corruption's sentinels 59901 .. 60000: no id is one
DEC_START = 3
GUARD_VALUE = 77
SLICE_ROWS = 65536
FILL4, FILL16 = -1, -5          # the fills of the two channels (gather and packer)
PACK_CHANNELS = {"c4": ("int32", FILL4), "c16": ("int64", FILL16, 2)}
PACK_REF_CHANNELS = [(np.int32, 1, FILL4), (np.int64, 2, FILL16)]
PRE, SUF, MID, END = 60001, 60002, 60003, 60004  # fill-in-the-middle's sentinels
CHAT_TPL = chat_ref.Template([[11, 12, 13], [21], []], [[14, 15], [22, 23], []], suffix_loss=[2, 1, 0], bos=BOS, eos=EOS)
CHAT_LOSS = 0b011


def side(pos, B):
    """which side of the boundary a flat position is on"""
    pos, B = int(pos), int(B)
    name = {W.B31: "2^31", W.B32: "2^32"}.get(B, str(B))
    if pos < B:
        return "below %s" % name
    return "at or past %s%s" % (name, ": negative as int32" if B == W.B31 else ": wraps as uint32" if B == W.B32 else "")


# ---- rows -----------------------------------------------------------------------------------------------------------
def rows_shape(B, L):
    return B // L + 64


def band(B, L):
    """rows [a, b) on both sides of flat element B (a >= 0)"""
    return max(0, B // L - 64), B // L + 64


def padded_docs(B, L, seed=9, long_len=5000, n_long=50):
    """-> (lens, offs, truncated rows, empty rows): the two lists name rows inside the band, one below and one past B each"""
    n = rows_shape(B, L)
    a, b = band(B, L)
    k = B // L
    assert 8 <= k and n == b and long_len + 2 > L
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, size=n)
    lens[rng.integers(0, n, size=n_long)] = long_len
    truncated, empty = [k - 3, k + 2], [k - 2, k + 3]
    lens[truncated] = long_len
    lens[empty] = 0
    lens[0], lens[k], lens[n - 1] = 17, 23, 31  # (row 0, the row that holds B and the last row differ in length)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return lens, offs, truncated, empty


def draw_ids(n, device="cpu", seed=5, lo=ID_LO, hi=ID_HI):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.randint(lo, hi, (n,), dtype=torch.int32, device=device, generator=g)


def gather_values(n, device="cpu"):
    """-> (int32 [n], int64 [n, 2]): records of 4 and 16 bytes that are a function of the token's index"""
    import torch
    i = torch.arange(n, dtype=torch.int64, device=device)
    return (i * 7 + 3).to(torch.int32), torch.stack((i * 3 + 1, -i - 2 ** 40), dim=1).contiguous()


def _sides(plan, L):
    """cols [1, L], in_a, in_b [n, L], end_b [n, 1] of a plan whose sides lie inside their rows"""
    import torch
    cols = torch.arange(L, dtype=torch.int64, device=plan.device)[None, :]
    ka, ca, kb, cb = (plan[:, i:i + 1] for i in (3, 4, 6, 7))
    in_a = (cols >= ca) & (cols < ca + ka)
    in_b = ~in_a & (cols >= cb) & (cols < cb + kb)
    return cols, in_a, in_b, cb + kb


def torch_lm_labels(ids, mask, plan, flags, ignore=IGN):
    """lm_labels of the rows given: flags of targets_ref.LABELS_*, LABELS_SHIFT among them"""
    import torch
    L = ids.shape[1]
    cols, in_a, in_b, end_b = _sides(plan, L)
    kind = torch.full(ids.shape, targets_ref.LABELS_END, dtype=torch.uint8, device=ids.device)
    kind[(cols < end_b).expand_as(kind)] = targets_ref.LABELS_TEMPLATE
    kind[in_b] = targets_ref.LABELS_B
    kind[in_a] = targets_ref.LABELS_A
    real = mask != 0
    loss = real & ((kind & (flags & 15)) != 0)
    ign = torch.full_like(ids, ignore)
    if flags & targets_ref.LABELS_SHIFT:
        out = ign.clone()
        out[:, :-1] = torch.where(real[:, :-1] & loss[:, 1:], ids[:, 1:], ign[:, 1:])
        return out
    return torch.where(loss, ids, ign)


def torch_gather(plan, L, values, fill):
    """gather_rows of a padded plan (one side): values [n] or [n, 2]"""
    import torch
    cols, in_a, _in_b, _end = _sides(plan, L)
    idx = (plan[:, 2:3] + (cols - plan[:, 4:5])).clamp_(0, max(values.shape[0] - 1, 0))
    v = values[idx]
    f = torch.full_like(v, fill)
    return torch.where(in_a if values.dim() == 1 else in_a[..., None], v, f)


def torch_packed_labels(values, seg, shift, ignore=IGN):
    import torch
    ign = torch.full_like(values, ignore)
    if not shift:
        return torch.where(seg != 0, values, ign)
    out = ign.clone()
    out[:, :-1] = torch.where((seg[:, 1:] == seg[:, :-1]) & (seg[:, :-1] != 0), values[:, 1:], ign[:, 1:])
    return out


def segment_rows(r0, r1, L, device="cpu"):
    """segment ids of rows [r0, r1) by a formula of (row, column): runs of 5 .. 15 columns, 0 .. 8 columns of padding (fewer than L)"""
    import torch
    r = torch.arange(r0, r1, dtype=torch.int64, device=device)[:, None]
    c = torch.arange(L, dtype=torch.int64, device=device)[None, :]
    seg = 1 + (c + r) // (5 + r % 11) - r // (5 + r % 11)
    return torch.where(c >= L - r % 9 % L, torch.zeros_like(seg), seg).to(torch.int32)


def _first(bad, r0, per_row, B, what, row_len=None):
    """raise for the first True of bad (rows from r0 on, per_row elements each; row_len: the elements of a row of the
    output where bad holds one value per row)"""
    import torch
    if bool(bad.any()):
        k = int(bad.reshape(-1).to(torch.uint8).argmax())
        r, j = r0 + k // per_row, k % per_row
        flat = r * (per_row if row_len is None else row_len) + j
        raise AssertionError("%s: row %d, element %d of the row, flat position %d, %s" % (what, r, j, flat, side(flat, B)))


def assert_rect(got, want_of, B, what, slice_rows=SLICE_ROWS):
    """got [n_rows, ...] against want_of(r0, r1) -> the rows [r0, r1) of the reference, slice_rows rows at a time"""
    n_rows = got.shape[0]
    per_row = got[0].numel() if n_rows else 1
    for r0 in range(0, n_rows, slice_rows):
        r1 = min(n_rows, r0 + slice_rows)
        want = want_of(r0, r1)
        assert want.shape == got[r0:r1].shape and want.dtype == got.dtype, (what, tuple(want.shape), want.dtype)
        _first(got[r0:r1] != want, r0, per_row, B, what + " differs from the reference")
        del want


def assert_band(got, want, a, B, what):
    """got[a:a + len(want)] (a torch tensor) against numpy rows of a Python reference"""
    import torch
    w = torch.from_numpy(np.ascontiguousarray(want)).to(got.device)
    g = got[a:a + w.shape[0]]
    assert g.shape == w.shape and g.dtype == w.dtype, (what, tuple(g.shape), tuple(w.shape), g.dtype, w.dtype)
    _first(g != w, a, g[0].numel() if len(g) else 1, B, what + " differs from the reference")


def cut(a, b, *tensors):
    return [None if t is None else t[a:b].cpu().numpy() for t in tensors]


def mlm_thresholds(p=0.15, mf=0.8, rf=0.1):
    mask_below = int(mf * 2 ** 32)
    return dict(select_below=int(p * 2 ** 32), mask_below=mask_below, random_below=min(2 ** 32, max(mask_below, int((mf + rf) * 2 ** 32))))


def mlm_band(ids, plan, a, b, *, seed, words=None, p=0.15):
    """targets_ref.mlm_ref on rows [a, b) -> (out, labels)"""
    i, pl = cut(a, b, ids, plan)
    w = None if words is None else words.cpu().numpy()
    out, labels, wrong = targets_ref.mlm_ref(i, pl, w, seed=seed, mask_id=MASK_ID, vocab_size=VOCAB, ignore_index=IGN, first_row=a,
                                             **mlm_thresholds(p))
    assert not wrong
    return out, labels


def span_band(ids, mask, plan, a, b, *, seed, density=0.15):
    """span_ref.span_corrupt_ref on rows [a, b) -> (out, out_mask, labels, in_len, tgt_len, dec)"""
    i, m, pl = cut(a, b, ids, mask, plan)
    res = span_ref.span_corrupt_ref(i, m, pl, seed=seed, sentinel_first=SENT_FIRST, n_sentinels=N_SENT, target_eos_id=EOS,
                                    decoder_start_id=DEC_START, pad_id=PAD, ignore_index=IGN, first_row=a, **span_ref.thresholds(density))
    assert not res[6]
    return res[:6]


def within_six_sigma(count, n, p, what, spread=1):
    """a count of n draws of probability p each; spread: the most draws that fall together (a word's tokens)"""
    bound = 6 * math.sqrt(spread * n * p * (1 - p)) + 1
    assert abs(count - n * p) <= bound, "%s: %d of %d, %.1f expected, more than %.1f off" % (what, count, n, n * p, bound)


def mlm_invariants(ids, plan, out, labels, B, *, p=0.15, mf=0.8, rf=0.1, words=None, word_len=1, slice_rows=SLICE_ROWS):
    """What holds of every element of a mask_tokens result whatever was drawn, and of the totals within six binomial
    standard deviations (a bound from the counts: the draws of different columns -- of different words in whole-word mode,
    hence word_len -- are independent).  -> the counts"""
    n_rows, L = ids.shape
    n_elig = n_sel = n_mask = n_rand = 0
    for r0 in range(0, n_rows, slice_rows):
        r1 = min(n_rows, r0 + slice_rows)
        i, o, l, pl = ids[r0:r1], out[r0:r1], labels[r0:r1], plan[r0:r1]
        cols, elig, _in_b, _end = _sides(pl, L)
        if words is not None:
            idx = (pl[:, 2:3] + (cols - pl[:, 4:5])).clamp_(0, words.numel() - 1)
            elig = elig & (words[idx] >= 0)  # a word below 0 protects its token
            del idx
        sel = l != IGN
        _first(sel & (l != i), r0, L, B, "labels is neither ignore_index nor the id")
        _first(~sel & (o != i), r0, L, B, "a column that was not selected was changed")
        _first(sel & ~elig, r0, L, B, "a column off the side's tokens (or a protected one) was selected")
        masked, rand = sel & (o == MASK_ID), sel & (o >= 0) & (o < VOCAB)
        _first(sel & ~masked & ~rand & (o != i), r0, L, B, "a selected column holds neither its id, nor the mask id, nor a random id")
        n_elig += int(elig.sum())
        n_sel += int(sel.sum())
        n_mask += int(masked.sum())
        n_rand += int(rand.sum())
        del cols, elig, sel, masked, rand
    within_six_sigma(n_sel, n_elig, p, "selected columns", word_len)
    if word_len == 1:
        within_six_sigma(n_mask, n_elig, p * mf, "columns that became the mask id")
        within_six_sigma(n_rand, n_elig, p * rf, "columns that became a random id")
    else:  # (the kind is drawn per column: independent given the selection)
        within_six_sigma(n_mask, n_sel, mf, "selected columns that became the mask id")
        within_six_sigma(n_rand, n_sel, rf, "selected columns that became a random id")
    return n_elig, n_sel, n_mask, n_rand


def span_invariants(mask, out, out_mask, labels, in_len, tgt_len, dec, B, slice_rows=SLICE_ROWS):
    """What holds of every row of a corrupt_spans result (L_tgt = L, a target eos, a decoder start) whatever was drawn."""
    import torch
    n_rows, L = mask.shape
    cols = torch.arange(L, dtype=torch.int64, device=mask.device)[None, :]
    for r0 in range(0, n_rows, slice_rows):
        r1 = min(n_rows, r0 + slice_rows)
        m, o, om, l, d = mask[r0:r1], out[r0:r1], out_mask[r0:r1], labels[r0:r1], dec[r0:r1]
        n_in, n_tgt = in_len[r0:r1].to(torch.int64), tgt_len[r0:r1].to(torch.int64)
        _first(om.sum(dim=1, dtype=torch.int64) != n_in, r0, 1, B, "out_mask.sum() is not input_lengths (per row)", row_len=L)
        _first(om != (cols < n_in[:, None]).to(om.dtype), r0, L, B, "the corrupted row is not compact")
        _first((om == 0) & (o != PAD), r0, L, B, "a column behind the corrupted row is not pad_id")
        _first((l != IGN).sum(dim=1) != torch.clamp(n_tgt, max=L), r0, 1, B, "the labels do not hold min(target_lengths, L) ids (per row)", row_len=L)
        runs = ((o > SENT_FIRST - N_SENT) & (o <= SENT_FIRST) & (om != 0)).sum(dim=1)
        _first(n_in - runs + (n_tgt - runs - 1) != (m != 0).sum(dim=1), r0, 1, B,
               "kept columns plus noise columns are not the real columns (per row)", row_len=L)
        _first(d[:, 0] != DEC_START, r0, 1, B, "decoder_input_ids does not begin with the start id (per row)", row_len=L)
        _first(d[:, 1:] != torch.where(l[:, :-1] == IGN, torch.full_like(l[:, :-1], PAD), l[:, :-1]), r0, L - 1, B,
               "decoder_input_ids is not labels moved right (element: of columns 1 .. L - 1)")


# ---- the packed stream ----------------------------------------------------------------------------------------------
class Stream:
    """lens, offs: the documents; sync: the documents that start at a row's first element (every sync_every-th);
    start(d): the stream position of document d (every document carries an eos)"""

    def __init__(self, lens, offs, L, sync_every, n_synced):
        self.lens, self.offs, self.L, self.sync_every = lens, offs, L, sync_every
        self.n_docs, self.n_ids = len(lens), int(offs[-1])
        self.total = self.n_ids + self.n_docs
        self.sync = list(range(0, n_synced + 1, sync_every))
        self.rows = self.total // L

    def start(self, d):
        return int(self.offs[d]) + d

    def band(self, B):
        """(d0, d1, row0, row1): the sync points either side of stream position B, the rows between them"""
        g = max(i for i, d in enumerate(self.sync) if self.start(d) <= B)
        d0, d1 = self.sync[g], self.sync[g + 1]
        return d0, d1, self.start(d0) // self.L, self.start(d1) // self.L

    def tail(self):
        """(d0, row0): the last sync point and its row -- the rows from there on, the flushed one included"""
        return self.sync[-1], self.start(self.sync[-1]) // self.L


def packed_stream(B, L, seed=3, sync_every=4096, extra=None, tail_docs=777):
    """Documents of 0 .. 64 ids (one in 512 of L .. 2 L: it covers whole rows) whose stream passes B + extra"""
    extra = 64 * L if extra is None else extra
    rng = np.random.default_rng(seed)
    groups = -(-(B + extra) // (sync_every * 38)) + 1
    while True:
        n = groups * sync_every
        lens = rng.integers(0, 65, size=n + tail_docs)
        long = rng.random(n + tail_docs) < 1 / 512
        lens[long] = rng.integers(L, 2 * L + 1, size=int(long.sum()))
        g = lens[:n].reshape(groups, sync_every)
        g[:, -1] += (-(g.sum(axis=1) + sync_every)) % L  # (the group's stream: its ids and an eos each)
        offs = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        s = Stream(lens, offs, L, sync_every, n)
        if s.start(n) >= B + extra:
            assert s.total % L, "the flushed row would be empty"
            return s
        groups += 1


def channel_values(i0, i1, device=None):
    """the two channels' records of ids [i0, i1): the low 31 bits of the flat index; (index, ~index).  device None: numpy"""
    if device is None:
        i = np.arange(i0, i1, dtype=np.int64)
        return (i & 0x7FFFFFFF).astype(np.int32), np.stack((i, ~i), axis=1)
    import torch
    i = torch.arange(i0, i1, dtype=torch.int64, device=device)
    return (i & 0x7FFFFFFF).to(torch.int32), torch.stack((i, ~i), dim=1).contiguous()


def packed_rows_ref(stream, ids_np, d0, d1, flush=False):
    """packed_ref.Packer fed documents [d0, d1) alone (ids_np: THEIR ids) -> its dict; flush: the flushed row appended"""
    i0, i1 = int(stream.offs[d0]), int(stream.offs[d1])
    assert len(ids_np) == i1 - i0 and stream.start(d0) % stream.L == 0
    p = packed_ref.Packer(stream.L, eos_id=EOS, pad_id=PAD, channels=PACK_REF_CHANNELS)
    parts = [p.add(ids_np, stream.offs[d0:d1 + 1] - i0, list(channel_values(i0, i1)))]
    if flush:
        parts.append(p.flush())
    return packed_ref.cat(parts)


def assert_packed_band(rows, want, row0, B, what):
    """rows: the packer's dict of torch tensors; want: packed_rows_ref's; from row row0 on"""
    for k in ("input_ids", "position_ids", "segment_ids"):
        assert_band(rows[k], want[k], row0, B, "%s, %s" % (what, k))
    for name, w in zip(PACK_CHANNELS, want["channels"]):
        assert_band(rows[name], w, row0, B, "%s, channel %s" % (what, name))


def packed_totals(parts, sum_ids, n_docs, n_ids, slice_rows=SLICE_ROWS):
    """Two values over all rows (parts: the dicts of add() and flush()), each from the input stream alone: the sum of
    input_ids is the ids' sum plus an eos per document (pad_id is 0); as many real columns as the stream is long."""
    import torch
    total = real = 0
    for rows in parts:
        for r0 in range(0, rows["input_ids"].shape[0], slice_rows):
            total += int(rows["input_ids"][r0:r0 + slice_rows].sum(dtype=torch.int64))
            real += int((rows["segment_ids"][r0:r0 + slice_rows] != 0).sum())
    assert PAD == 0
    assert (total, real) == (sum_ids + EOS * n_docs, n_ids + n_docs), \
        "sum of input_ids %d, %d expected; %d real columns, the stream has %d" % (total, sum_ids + EOS * n_docs, real, n_ids + n_docs)


# ---- copies of a block: chat, fill-in-the-middle of pieces ----------------------------------------------------------------
def assert_copies(got, row, R, step, B, what, slice_elems=2 ** 26):
    """got[r * T + j] == row[j] + (r * step where row[j] >= 0) for every copy r < R (T = len(row)), compared on got's
    device in slices.  step 0: every copy equals the row; step n_ids_block: the source."""
    import torch
    row = torch.from_numpy(np.ascontiguousarray(row)).to(got.device)
    T = row.numel()
    assert got.numel() == R * T and got.dtype == row.dtype, "%s: %d elements of %s, %d copies of %d expected" % (what, got.numel(), got.dtype, R, T)
    moves = (row >= 0).to(row.dtype) * step
    per = max(1, slice_elems // max(T, 1))
    for r0 in range(0, R, per):
        r1 = min(R, r0 + per)
        want = row[None, :] + torch.arange(r0, r1, dtype=row.dtype, device=row.device)[:, None] * moves[None, :] if step else row[None, :]
        ne = got[r0 * T:r1 * T].view(r1 - r0, T) != want
        if bool(ne.any()):
            k = int(ne.reshape(-1).to(torch.uint8).argmax())
            r, j = r0 + k // T, k % T
            raise AssertionError("%s: copy %d, element %d of the copy, flat position %d, %s: %d, the block has %d%s"
                                 % (what, r, j, r * T + j, side(r * T + j, B), int(got[r * T + j]), int(row[j]),
                                    " + %d x %d" % (r, step) if step and int(row[j]) >= 0 else ""))
        del ne, want


def assert_copy_offsets(got, oo_block, R, B, what):
    """got[r * n + d] == oo_block[d] + r * T, got[R * n] == R * T (T = oo_block[n])"""
    n, T = len(oo_block) - 1, int(oo_block[-1])
    assert got.numel() == R * n + 1
    assert int(got[R * n]) == R * T, "%s: the total is %d, %d copies of %d expected" % (what, int(got[R * n]), R, T)
    assert_copies(got[:R * n], np.asarray(oo_block[:-1], dtype=np.int64), R, T, B, what)


def _conv(turns):
    """[(role, n ids)] -> rendered length"""
    return 2 + sum(len(CHAT_TPL.prefix[r]) + n + len(CHAT_TPL.suffix[r]) for r, n in turns)


class ChatBlock:
    """turns: [(role, n)] per conversation -> ids, offsets, roles, conv (numpy) and chat_ref's render of them"""

    def __init__(self, convs, seed, lo, hi):
        rng = np.random.default_rng(seed)
        lens = [n for c in convs for _r, n in c]
        self.roles = np.array([r for c in convs for r, _n in c], dtype=np.int32)
        self.offsets = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=self.offsets[1:])
        self.conv = np.zeros(len(convs) + 1, dtype=np.int64)
        np.cumsum([len(c) for c in convs], out=self.conv[1:])
        self.ids = rng.integers(1000, 50000, size=int(self.offsets[-1])).astype(np.int32)
        self.n_ids, self.n_turns, self.n_conv = len(self.ids), len(lens), len(convs)
        self.ref = chat_ref.render(CHAT_TPL, self.ids, self.offsets, self.roles, self.conv, loss_roles=CHAT_LOSS, ignore_index=IGN)
        assert self.ref["err"] == 0
        self.n_out = len(self.ref["out_ids"])
        self.lo, self.hi, self.p_lo, self.p_hi = lo, hi, lo % self.n_out, hi % self.n_out


def _fill_convs(convs, rng, size, target):
    """random conversations, then one of a single bare turn, up to rendered length `target` exactly"""
    assert target - size >= 2
    while target - size > 3000:
        turns = [(rng.randrange(3), rng.choice((0, 0, 1, 7, 40, 200, rng.randrange(300)))) for _ in range(rng.randrange(0, 7))]
        convs.append(turns)
        size += _conv(turns)
    convs.append([(2, target - size - 2)])  # role 2 has neither prefix nor suffix: n ids render as bos + n + eos
    return target


CHAT_ZONE = [(0, 0), (1, 50), (2, 0), (0, 9)]  # behind p: bos, an empty turn of role 0 (prefix, suffix), a turn start at p + 6


def chat_block(lo, hi, around=2 ** 20, seed=1, room=8192):
    """A block of rendered length n_out (odd, >= around) with a conversation's eos at p - 1 and CHAT_ZONE from p on, for
    p = lo mod n_out and hi mod n_out"""
    rng = random.Random(seed)
    n_out = W.choose_length(around + 1, lo, hi, room, room)
    convs, size = [], 0
    for p in sorted((lo % n_out, hi % n_out)):
        size = _fill_convs(convs, rng, size, p)
        convs.append(list(CHAT_ZONE))
        size += _conv(CHAT_ZONE)
    _fill_convs(convs, rng, size, n_out)
    b = ChatBlock(convs, seed, lo, hi)
    assert b.n_out == n_out
    check_chat_layout(b)
    return b


def check_chat_layout(b):
    """what chat_block() claims, from the render alone"""
    r = b.ref
    assert b.n_out % 2 == 1
    for p in (b.p_lo, b.p_hi):
        i = int(np.searchsorted(r["out_offsets"], p))
        assert r["out_offsets"][i] == p, "no conversation starts at p"
        assert r["out_ids"][p - 1] == EOS and r["turn_ids"][p - 1] == -1, "no tail in front of p"
        assert r["out_ids"][p] == BOS and r["turn_ids"][p] == -1, "no bos at p"
        t = int(b.conv[i])
        assert b.offsets[t + 1] == b.offsets[t] and b.roles[t] == 0, "the conversation at p does not begin with an empty turn"
        assert r["out_ids"][p + 1:p + 6].tolist() == [11, 12, 13, 14, 15] and (r["turn_ids"][p + 1:p + 6] == 0).all()
        assert r["turn_ids"][p + 6] == 1 and r["out_ids"][p + 6] == 21, "no turn start at p + 6"
        assert r["source"][p + 7] >= 0 and r["labels"][p + 7] == r["out_ids"][p + 7]


class FimBlock:
    """pieces: [(prefix, middle, suffix lengths)] per document, kinds periodic (document d: d mod 3) -> ids, piece offsets,
    kinds and fim_ref's render"""

    def __init__(self, pieces, seed, lo, hi):
        rng = np.random.default_rng(seed)
        flat = [n for doc in pieces for n in doc]
        self.offsets = np.zeros(len(flat) + 1, dtype=np.int64)
        np.cumsum(flat, out=self.offsets[1:])
        self.kinds = (np.arange(len(pieces)) % 3).astype(np.int32)
        self.ids = rng.integers(1000, 50000, size=int(self.offsets[-1])).astype(np.int32)
        self.n_ids, self.n_docs = len(self.ids), len(pieces)
        self.plan = fim_ref.plan_pieces(self.offsets)
        self.ref = fim_ref.render(self.ids, self.plan, self.kinds, pre=PRE, suf=SUF, mid=MID, end=END, loss_parts=fim_ref.LOSS_MIDDLE,
                                  ignore_index=IGN)
        self.n_out = len(self.ref["out_ids"])
        self.lo, self.hi, self.p_lo, self.p_hi = lo, hi, lo % self.n_out, hi % self.n_out


def _fim_len(d, doc):
    return sum(doc) + (4 if d % 3 else 0)


def _fill_pieces(pieces, rng, size, target):
    """random documents, then a plain one (its number is a multiple of 3) up to rendered length `target` exactly"""
    while target - size > 3000 or len(pieces) % 3:
        doc = tuple(rng.choice((0, 0, 1, 5, 60, rng.randrange(200))) for _ in range(3))
        size += _fim_len(len(pieces), doc)
        pieces.append(doc)
    assert target >= size
    pieces.append((target - size, 0, 0))
    return target


FIM_ZONE = (7, 20, 30)  # a PSM document from p - 10 on: the suffix sentinel at p - 2, the suffix across p


def fim_block(lo, hi, around=2 ** 20, seed=2, room=8192):
    rng = random.Random(seed)
    n_out = W.choose_length(around + 1, lo, hi, room, room)
    pieces, size = [], 0
    for p in sorted((lo % n_out, hi % n_out)):
        size = _fill_pieces(pieces, rng, size, p - 10)
        assert len(pieces) % 3 == 1
        pieces.append(FIM_ZONE)
        size += _fim_len(1, FIM_ZONE)
    _fill_pieces(pieces, rng, size, n_out)
    b = FimBlock(pieces, seed, lo, hi)
    assert b.n_out == n_out
    check_fim_layout(b)
    return b


def check_fim_layout(b):
    r = b.ref
    assert b.n_out % 2 == 1
    for p in (b.p_lo, b.p_hi):
        d = int(np.searchsorted(r["out_offsets"], p - 10, side="right")) - 1
        assert r["out_offsets"][d] == p - 10 and b.kinds[d] == fim_ref.PSM and b.plan[d].tolist()[1:] == [57, 7, 27]
        assert r["out_ids"][p - 10] == PRE and r["out_ids"][p - 2] == SUF and r["parts"][p - 1] == r["parts"][p] == fim_ref.PART_SUFFIX
        assert r["source"][p - 3] + 21 == r["source"][p - 1], "the suffix does not begin behind the middle"


def copies(block_offsets, per_copy, R, device):
    """the offsets of R copies, on the device"""
    import torch
    return torch.from_numpy(W.repeated_offsets(block_offsets, per_copy, R)).to(device)


# ---- fill-in-the-middle at token level ------------------------------------------------------------------------------------
FIM_SEED, FIM_FB, FIM_SB = 11, 2 ** 31, 2 ** 31


def fim_docs(B, seed=4, extra=2 ** 16, mean=200):
    """lens, offs of documents of 0 .. 2 mean ids (one in 300 of 3000 .. 6000) whose ids pass B + extra"""
    rng = np.random.default_rng(seed)
    n = (B + extra) // mean + 1
    while True:
        lens = rng.integers(0, 2 * mean + 1, size=n)
        long = rng.random(n) < 1 / 300
        lens[long] = rng.integers(3000, 6001, size=int(long.sum()))
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        if offs[-1] >= B + extra:
            return lens, offs
        n += n // 50 + 1


def fim_band(ids_np, offs, d0, d1):
    """fim_ref.fim_tokens on documents [d0, d1) (ids_np: THEIR ids), first_doc = d0, with source and the plan's src0 moved
    to the batch's ids -> its dict"""
    i0 = int(offs[d0])
    r = fim_ref.fim_tokens(ids_np, np.asarray(offs[d0:d1 + 1]) - i0, seed=FIM_SEED, fim_below=FIM_FB, spm_below=FIM_SB, first_doc=d0,
                           pre=PRE, suf=SUF, mid=MID, end=END, loss_parts=fim_ref.LOSS_MIDDLE, ignore_index=IGN)
    r["source"] = np.where(r["source"] >= 0, r["source"] + i0, -1)
    r["plan"] = r["plan"].copy()
    r["plan"][:, 0] += i0
    return r


def assert_fim_band(got, want, d0, d1, B):
    """got: dict of torch tensors (out_ids, labels, parts, source, out_offsets, plan [n, 4], kinds) of the whole batch"""
    oo = got["out_offsets"]
    o0, o1 = int(oo[d0]), int(oo[d1])
    assert o1 - o0 == len(want["out_ids"]), "documents %d .. %d render %d elements, the reference %d" % (d0, d1, o1 - o0, len(want["out_ids"]))
    rel = (oo[d0:d1 + 1] - o0).cpu().numpy()
    bad = np.nonzero(rel != want["out_offsets"])[0]
    assert bad.size == 0, "out_offsets of document %d (ids from %d on, %s)" % (d0 + bad[0], int(want["plan"][min(bad[0], d1 - d0 - 1), 0]), side(want["plan"][min(bad[0], d1 - d0 - 1), 0], B))
    for k in ("kinds", "plan"):
        g = got[k][d0:d1].cpu().numpy()
        bad = np.nonzero((g != want[k]).reshape(d1 - d0, -1).any(axis=1))[0]
        assert bad.size == 0, "%s of document %d: %s, the reference has %s" % (k, d0 + bad[0], g[bad[0]].tolist(), want[k][bad[0]].tolist())
    for k in ("out_ids", "labels", "parts", "source"):
        g = got[k][o0:o1].cpu().numpy()
        bad = np.nonzero(g != want[k])[0]
        assert bad.size == 0, "%s at output position %d (%s): %d, the reference has %d" % (k, o0 + bad[0], side(o0 + bad[0], B), g[bad[0]], want[k][bad[0]])


def fim_totals(got, offs_t, ids, n_ids, slice_elems=2 ** 27):
    """Over the whole batch, on its device: out_offsets is the documents' offsets plus four sentinels per transformed
    document in front; the total; the sum of out_ids is the ids' sum plus the sentinels'.  (An end sentinel: 4 per document.)"""
    import torch
    moved = got["kinds"] != fim_ref.PLAIN
    n_moved = int(moved.sum())
    before = torch.cumsum(moved.to(torch.int64), 0) - moved.to(torch.int64)
    want_oo = offs_t[:-1] + 4 * before
    bad = torch.nonzero(got["out_offsets"][:-1] != want_oo)
    assert bad.numel() == 0, "out_offsets[%d] is %d, not offsets + 4 x the transformed documents in front = %d" % (
        int(bad[0]), int(got["out_offsets"][int(bad[0])]), int(want_oo[int(bad[0])]))
    total = int(got["out_offsets"][-1])
    assert total == n_ids + 4 * n_moved, "out_offsets[-1] = %d, %d ids and %d transformed documents" % (total, n_ids, n_moved)
    s_in = sum(int(ids[a:a + slice_elems].sum(dtype=torch.int64)) for a in range(0, n_ids, slice_elems))
    s_out = sum(int(got["out_ids"][a:min(total, a + slice_elems)].sum(dtype=torch.int64)) for a in range(0, total, slice_elems))
    assert s_out == s_in + (PRE + SUF + MID + END) * n_moved, "the sum of out_ids is %d, %d expected" % (s_out, s_in + (PRE + SUF + MID + END) * n_moved)
    return n_moved


# ---- guard bands on the device ----------------------------------------------------------------------------------------
def guarded(n, dtype, device, guard=64):
    """n elements with a guard band on either side -> (the elements, the store).  (The guarded helpers of the features'
    own test files copy the store to the host, which a buffer of 2^31 elements does not allow.)"""
    import torch
    store = torch.empty(guard + n + guard, dtype=dtype, device=device)
    store[:guard] = GUARD_VALUE
    store[guard + n:] = GUARD_VALUE
    return store[guard:guard + n], store


def untouched(store, n, guard=64):
    return bool((store[:guard] == GUARD_VALUE).all()) and bool((store[guard + n:] == GUARD_VALUE).all())
