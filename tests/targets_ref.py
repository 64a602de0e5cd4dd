"""Training targets in plain numpy: the definitions that k_rows_mlm and k_rows_labels of csrc/hutk_collate.hip are
tested against (the rules are stated in full in include/hutoken_amd.h).

Philox4x32-10 is restated over uint64 arrays; mlm_ref and labels_ref decide every column of every row from the plan
alone, element by element, with the clipping rules of the gather (test_gpu_features.hostile_reference): a side is
clipped to the row, a negative length counts as 0, a column both sides claim is A's, a word outside its array is not
read."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SIDE_A, SIDE_B = 1, 2
LABELS_A, LABELS_B, LABELS_TEMPLATE, LABELS_END, LABELS_SHIFT = 1, 2, 4, 8, 16
COLUMN, WORD_A, WORD_B = 0, 1, 2  # the purposes of a draw


def philox4x32_10(counter, key):
    """counter: four and key: two arrays (or ints) of 32-bit values, broadcast together -> four uint64 arrays < 2**32"""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in np.broadcast_arrays(*counter, *key)]
    c0, c1, c2, c3, k0, k1 = c
    for _round in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return c0, c1, c2, c3


def draw(seed, row, unit, purpose):
    """key = (low32(seed), high32(seed)), counter = (low32(row), high32(row), unit, purpose)"""
    row = np.asarray(row, dtype=np.uint64)
    return philox4x32_10((row & MASK32, row >> np.uint64(32), unit, purpose), (seed & 0xFFFFFFFF, seed >> 32))


def threshold(p):
    return int(p * 2**32)


def clip_side(col, k, L):
    """one side of one plan -> (lo, hi, wrong): columns [lo, hi) of the row are the side's; lo == hi: none"""
    wrong = k < 0
    if k <= 0:
        return 0, 0, wrong
    if col < 0 or col >= L or k > L - col:
        wrong = True
    if col >= L or col <= -L:
        return 0, 0, wrong
    end = col + min(k, L)
    if end <= 0:
        return 0, 0, wrong
    return max(col, 0), min(end, L), wrong


def plan_sides(plan, L):
    """The sides of every row of a plan, clipped -> (in_a, in_b: bool [n_rows, L], end_b [n_rows, 1]: col_b + kb inside
    [0, L], wrong).  The plan is walked row by row in Python ints: a hostile entry is any int64."""
    n = len(plan)
    lo_a, hi_a, lo_b, hi_b, end_b = (np.zeros((n, 1), dtype=np.int64) for _ in range(5))
    wrong = False
    for r, (_item, _start, _sa, ka, ca, _sb, kb, cb) in enumerate(np.asarray(plan).tolist()):
        lo_a[r], hi_a[r], wrong_a = clip_side(ca, ka, L)
        lo_b[r], hi_b[r], wrong_b = clip_side(cb, kb, L)
        wrong |= wrong_a or wrong_b or bool(lo_a[r] < hi_a[r] and lo_b[r] < hi_b[r] and lo_b[r] < hi_a[r] and lo_a[r] < hi_b[r])
        end_b[r] = min(max(min(max(cb, -L), L) + min(max(kb, 0), 2 * L), 0), L)
    cols = np.arange(L)[None, :]
    in_a = (cols >= lo_a) & (cols < hi_a)
    in_b = ~in_a & (cols >= lo_b) & (cols < hi_b)  # a column both sides claim is A's
    return in_a, in_b, end_b, wrong


def mlm_ref(ids_rows, plan, words_a=None, words_b=None, *, seed, select_below, mask_below, random_below, mask_id,
            vocab_size=1, ignore_index=-100, sides=SIDE_A | SIDE_B, first_row=0):
    """ids_rows [n_rows, L], plan [n_rows, 8]; words_a None: token mode; words_b None: both sides read words_a.
    first_row: the number of the first row (a draw is a function of the row's number).
    -> (out, labels, wrong): wrong when the kernel must report HUTK_E_ARG."""
    ids_rows, plan = np.asarray(ids_rows), np.asarray(plan).reshape(-1, 8)
    n_rows, L = ids_rows.shape
    out = ids_rows.copy()
    labels = np.full_like(ids_rows, ignore_index)
    if words_a is not None and words_b is None:
        words_b = words_a
    in_a, in_b, _end_b, wrong = plan_sides(plan, L)
    selected = np.zeros((n_rows, L), dtype=bool)
    far = 2**40  # (an index beyond it is outside any array, and stays so with a column's distance added)
    for on, side_bit, src, col, words, purpose in ((in_a, SIDE_A, plan[:, 2], plan[:, 4], words_a, WORD_A),
                                                   (in_b, SIDE_B, plan[:, 5], plan[:, 7], words_b, WORD_B)):
        if not sides & side_bit:
            continue
        r, c = np.nonzero(on)  # the eligible columns of this side, one by one
        if words is None:
            selected[r, c] = draw(seed, first_row + r, c, COLUMN)[0] < select_below
            continue
        idx = np.clip(src, -far, far)[r] + (c - col[r])  # (col: of a side with columns |col| < L)
        inside = (idx >= 0) & (idx < len(words))  # a word outside its array is not read
        wrong |= bool((~inside).any())
        r, c, idx = r[inside], c[inside], idx[inside]
        w = np.asarray(words)[idx].astype(np.int64)
        r, c, w = r[w >= 0], c[w >= 0], w[w >= 0]  # a word below 0 protects its token
        selected[r, c] = draw(seed, first_row + r, w, purpose)[0] < select_below
    r, c = np.nonzero(selected)
    _u0, u1, u2, _u3 = draw(seed, first_row + r, c, COLUMN)
    labels[r, c] = ids_rows[r, c]
    random_ids = ((u2 * np.uint64(vocab_size)) >> np.uint64(32)).astype(ids_rows.dtype)
    masked, random = u1 < mask_below, (u1 >= mask_below) & (u1 < random_below)
    out[r[masked], c[masked]] = mask_id
    out[r[random], c[random]] = random_ids[random]
    return out, labels, wrong


def labels_ref(ids_rows, mask, plan, flags, ignore_index=-100):
    """-> (labels, wrong)"""
    ids_rows, mask = np.asarray(ids_rows), np.asarray(mask)
    n_rows, L = ids_rows.shape
    labels = np.full_like(ids_rows, ignore_index)
    in_a, in_b, end_b, wrong = plan_sides(np.asarray(plan).reshape(-1, 8), L)
    cols = np.arange(L)[None, :]
    kind = np.where(in_a, LABELS_A, np.where(in_b, LABELS_B, np.where(cols < end_b, LABELS_TEMPLATE, LABELS_END)))
    real = mask != 0
    loss = real & ((kind & flags) != 0)
    if flags & LABELS_SHIFT:  # what column c predicts; the last column predicts nothing
        hit = real[:, :-1] & loss[:, 1:]
        labels[:, :-1][hit] = ids_rows[:, 1:][hit]
    else:
        labels[loss] = ids_rows[loss]
    return labels, wrong
