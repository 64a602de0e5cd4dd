"""Training targets on the GPU (csrc/hutk_collate.hip: k_rows_mlm, k_rows_labels) against the numpy restatement of
tests/targets_ref.py, every comparison exact and over every element, for int32 and int64 rows.

The rows and their plans are the library's own (collate_* with return_plan=True) over random ids; the word ids of the
whole-word cases are made here (non-decreasing from 0 in every document, as token_word_ids_device gives them), those of
the end-to-end cases are the library's under the gpt2 preset.  Needs a real MI355X."""
import itertools

import numpy as np
import pytest

import features_cases as FC
import targets_ref as T

pytestmark = pytest.mark.gpu

E_ARG = 4
MASK_ID, VOCAB = 50264, 50257
WIDTHS = ("int32", "int64")
NAMES = {T.LABELS_A: "a", T.LABELS_B: "b", T.LABELS_TEMPLATE: "template", T.LABELS_END: "end"}
SUBSETS = [sum(c) for n in range(1, 5) for c in itertools.combinations(NAMES, n)]  # the 15 sets of selecting flags


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def host(t):
    return t.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def ragged(lens, rng, base=0):
    offs = np.full(len(lens) + 1, base, dtype=np.int64)
    offs[1:] += np.cumsum(lens, dtype=np.int64)
    return rng.integers(0, 50000, size=int(offs[-1])).astype(np.int32), offs


def words_of(offs, rng, n=None):
    """Word ids as token_word_ids_device gives them: in every document they begin at 0 and grow by 0 or 1 a token."""
    w = np.zeros(int(offs[-1]) if n is None else n, dtype=np.int32)
    for a, b in zip(offs[:-1], offs[1:]):
        if b > a:
            steps = rng.integers(0, 2, size=int(b - a))
            steps[0] = 0
            w[a:b] = np.cumsum(steps)
    return w


def thresholds(p, mf, rf):
    return dict(select_below=T.threshold(p), mask_below=T.threshold(mf), random_below=min(2**32, T.threshold(mf + rf)))


def check_mlm(ids_t, plan_t, *, seed, p=0.15, mf=0.8, rf=0.1, words=None, words_b=None, sides="both", ignore=-100, vocab=VOCAB):
    """mask_tokens against the restatement -> (out, labels) on the host"""
    import hutoken_amd
    kw = dict(word_ids=None if words is None else dev(words), word_ids_b=None if words_b is None else dev(words_b))
    out, labels = hutoken_amd.mask_tokens(ids_t, plan_t, mask_id=MASK_ID, vocab_size=vocab, seed=seed, mlm_probability=p,
                                          mask_fraction=mf, random_fraction=rf, sides=sides, ignore_index=ignore, check=True, **kw)
    assert out.dtype == ids_t.dtype and labels.dtype == ids_t.dtype and out.data_ptr() != ids_t.data_ptr()
    want = T.mlm_ref(host(ids_t), host(plan_t), words, words_b, seed=seed, mask_id=MASK_ID, vocab_size=vocab or 1, ignore_index=ignore,
                     sides={"a": 1, "b": 2, "both": 3}[sides], **thresholds(p, mf, rf))
    assert not want[2]
    got = host(out), host(labels)
    assert same(got[0], want[0]) and same(got[1], want[1]), (ids_t.shape, sides, seed)
    return got


def check_labels(ids_t, mask_t, plan_t, flags, ignore=-100):
    import hutoken_amd
    loss_on = tuple(NAMES[b] for b in NAMES if flags & b)
    got = hutoken_amd.lm_labels(ids_t, mask_t, plan_t, loss_on=loss_on, shift=bool(flags & T.LABELS_SHIFT), ignore_index=ignore, check=True)
    want, wrong = T.labels_ref(host(ids_t), host(mask_t), host(plan_t), flags, ignore)
    assert not wrong and got.dtype == ids_t.dtype and same(host(got), want), (ids_t.shape, flags)
    return want


def padded(lens, L, dtype, rng, **kw):
    import hutoken_amd
    ids, offs = ragged(lens, rng)
    res = hutoken_amd.collate_padded(dev(ids), dev(offs), L, dtype=dtype, return_plan=True, check=True, **kw)
    return res, ids, offs


# ---- tile edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [1, 3, 4, 7, 8, 16, 512, 4096, 4097, 8195])
def test_row_lengths(L, dtype):
    """1 .. 16: many rows per workgroup (300 rows are more than one holds); 512: eight rows per workgroup; 4096: one row
    per workgroup; 4097 and 8195: column chunks with a ragged last one.  3, 7, 4097 and 8195 take the path of one column
    per thread.  Either padding side, either truncation side; token and whole-word mode; labels with and without shift."""
    rng = np.random.default_rng(L)
    n = 300 if L <= 16 else 20 if L == 512 else 3
    tpl = dict(bos_id=50256, eos_id=50255) if L >= 3 else {}
    lens = [L + 5, 0, max(L - 3, 0)] + list(rng.integers(0, 2 * L + 2, size=n - 3))
    for side, tr in (("right", "left"), ("left", "right")):
        (ids_t, mask_t, lengths, plan_t), ids, offs = padded(lens, L, dtype, rng, padding_side=side, truncation=tr, pad_id=7, **tpl)
        assert ids_t.shape == (n, L) and int(lengths.max()) == L
        _out, labels = check_mlm(ids_t, plan_t, seed=L, p=0.3)
        if L >= 8:
            assert (labels != -100).any() and (labels == -100).any()
        check_mlm(ids_t, plan_t, seed=L + 1, p=0.5, words=words_of(offs, rng))
        for flags in (15, 15 | T.LABELS_SHIFT, T.LABELS_A | T.LABELS_SHIFT):
            check_labels(ids_t, mask_t, plan_t, flags)


@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [4, 16])
def test_row_counts(L, dtype):
    """A workgroup holds 256 rows of 4 or of 16 columns: one row, one short of a workgroup, a whole one, one more."""
    rng = np.random.default_rng(100 + L)
    for n in (1, 255, 256, 257):
        (ids_t, mask_t, _lengths, plan_t), _ids, offs = padded(list(rng.integers(0, L + 3, size=n)), L, dtype, rng, eos_id=2, pad_id=7)
        check_mlm(ids_t, plan_t, seed=n, p=0.4)
        check_mlm(ids_t, plan_t, seed=n, p=0.4, words=words_of(offs, rng))
        check_labels(ids_t, mask_t, plan_t, 15 | T.LABELS_SHIFT)
        check_labels(ids_t, mask_t, plan_t, T.LABELS_END)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_no_rows(dtype):
    import torch
    import hutoken_amd
    res = hutoken_amd.collate_padded(dev(np.zeros(0, np.int32)), dev(np.zeros(1, np.int64)), 8, dtype=dtype, return_plan=True)
    out, labels = hutoken_amd.mask_tokens(res[0], res[3], mask_id=1, vocab_size=5, seed=1, check=True)
    assert out.shape == (0, 8) and labels.shape == (0, 8) and labels.dtype == res[0].dtype
    out, labels = hutoken_amd.mask_tokens(res[0], res[3], mask_id=1, vocab_size=5, seed=1, word_ids=torch.zeros(0, dtype=torch.int32, device="cuda:0"))
    assert out.shape == (0, 8)
    assert hutoken_amd.lm_labels(res[0], res[1], res[3], check=True).shape == (0, 8)
    # documents without ids: rows of template and padding, nothing to select
    res = hutoken_amd.collate_padded(dev(np.zeros(0, np.int32)), dev(np.zeros(4, np.int64)), 8, eos_id=2, pad_id=7, dtype=dtype, return_plan=True)
    out, labels = hutoken_amd.mask_tokens(res[0], res[3], mask_id=1, vocab_size=5, seed=1, mlm_probability=1.0,
                                          word_ids=torch.zeros(0, dtype=torch.int32, device="cuda:0"), check=True)
    assert same(host(out), host(res[0])) and bool((labels == -100).all())
    assert host(hutoken_amd.lm_labels(res[0], res[1], res[3], check=True)).tolist() == [[2] + [-100] * 7] * 3


# ---- paths ------------------------------------------------------------------------------------------------------------
def raw_mlm(plan, ids, out, labels, L, width, words=None, seed=5, p=0.5, sides=3, ignore=-100):
    """hutk_rows_mlm_device on tensors as they are (views included) -> the error word"""
    import torch
    from hutoken_amd import _capi
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    th = thresholds(p, 0.8, 0.1)
    _capi.rows_mlm_device(plan.data_ptr(), plan.shape[0], L, ids.data_ptr(), width, 0 if words is None else words.data_ptr(),
                          0 if words is None else words.numel(), 0, 0, seed, th["select_below"], th["mask_below"], th["random_below"],
                          MASK_ID, VOCAB, ignore, sides, out.data_ptr(), labels.data_ptr(), err.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return int(err.item())


def raw_labels(plan, ids, mask, labels, L, width, flags, ignore=-100):
    import torch
    from hutoken_amd import _capi
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    _capi.rows_labels_device(plan.data_ptr(), plan.shape[0], L, ids.data_ptr(), width, mask.data_ptr(), flags, ignore,
                             labels.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return int(err.item())


def view_at(t, off, fill=77):
    """a copy of t (flat) that begins `off` elements behind a 16-byte boundary, and the store around it"""
    import torch
    store = torch.full((t.numel() + 8,), fill, dtype=t.dtype, device="cuda:0")
    v = store[off:off + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == off * t.element_size() % 16
    return v, store


@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [8, 4100])
def test_views_off_the_16_byte_boundary(L, dtype):
    """Each of the rectangles one element behind a 16-byte boundary, the others on one: the path of one column per thread,
    with the result of the aligned path and nothing written around the outputs."""
    import torch
    rng = np.random.default_rng(L)
    n = 300 if L == 8 else 2
    (ids_t, mask_t, _lengths, plan_t), _ids, offs = padded(list(rng.integers(0, L + 3, size=n)), L, dtype, rng, bos_id=1, pad_id=7)
    width = ids_t.element_size()
    words = words_of(offs, rng)
    for w in (None, words):
        want = T.mlm_ref(host(ids_t), host(plan_t), w, seed=5, mask_id=MASK_ID, vocab_size=VOCAB, **thresholds(0.5, 0.8, 0.1))
        for off_i, off_o, off_l in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            (vi, _si), (vo, so), (vl, sl) = view_at(ids_t, off_i), view_at(torch.zeros_like(ids_t), off_o), view_at(torch.zeros_like(ids_t), off_l)
            assert raw_mlm(plan_t, vi, vo, vl, L, width, None if w is None else dev(w)) == 0
            assert same(host(vo).reshape(n, L), want[0]) and same(host(vl).reshape(n, L), want[1]), (off_i, off_o, off_l)
            for store, off in ((so, off_o), (sl, off_l)):
                rest = host(store)
                assert (rest[:off] == 77).all() and (rest[off + n * L:] == 77).all()
    flags = 15 | T.LABELS_SHIFT
    want, _w = T.labels_ref(host(ids_t), host(mask_t), host(plan_t), flags)
    for off_i, off_m, off_l in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 3, 1)):
        (vi, _si), (vm, _sm), (vl, sl) = view_at(ids_t, off_i), view_at(mask_t, off_m), view_at(torch.zeros_like(ids_t), off_l)
        assert raw_labels(plan_t, vi, vm, vl, L, width, flags) == 0
        assert same(host(vl).reshape(n, L), want), (off_i, off_m, off_l)
        rest = host(sl)
        assert (rest[:off_l] == 77).all() and (rest[off_l + n * L:] == 77).all()


@pytest.mark.parametrize("dtype", WIDTHS)
def test_in_place_equals_out_of_place(dtype):
    import hutoken_amd
    rng = np.random.default_rng(11)
    for L in (16, 7, 4100):
        n = 300 if L < 100 else 2
        (ids_t, _m, _l, plan_t), _ids, offs = padded(list(rng.integers(0, L + 3, size=n)), L, dtype, rng, eos_id=2, pad_id=7)
        for w in (None, dev(words_of(offs, rng))):
            kw = dict(mask_id=MASK_ID, vocab_size=VOCAB, seed=3, mlm_probability=0.5, word_ids=w, check=True)
            out, labels = hutoken_amd.mask_tokens(ids_t, plan_t, **kw)
            mine = ids_t.clone()
            out2, labels2 = hutoken_amd.mask_tokens(mine, plan_t, inplace=True, **kw)
            assert out2.data_ptr() == mine.data_ptr() and same(host(mine), host(out)) and same(host(labels2), host(labels))
            assert not same(host(out), host(ids_t))


# ---- layouts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
def test_windows_with_words_across_their_edges(dtype):
    import hutoken_amd
    rng = np.random.default_rng(12)
    L, stride = 16, 4
    ids, offs = ragged([0, 14, 15, 100, 3, 41] + list(rng.integers(0, 60, size=150)), rng)
    words = words_of(offs, rng)
    straddles = 0
    for side in ("right", "left"):
        res = hutoken_amd.collate_windows(dev(ids), dev(offs), L, stride, bos_id=1, eos_id=2, pad_id=7, padding_side=side, dtype=dtype,
                                          return_plan=True, check=True)
        ids_t, mask_t, plan_t = res[0], res[1], res[4]
        plan = host(plan_t)
        assert len(plan) > 256
        _out, labels = check_mlm(ids_t, plan_t, seed=21, p=0.5, words=words)
        check_mlm(ids_t, plan_t, seed=22, p=0.3)
        for r, (_item, _start, src, k, col, _sb, _kb, _cb) in enumerate(plan.tolist()):
            w, sel = words[src:src + k], labels[r, col:col + k] != -100
            for word in np.unique(w):  # a word is selected wholly or not at all, within its row
                assert len(set(sel[w == word].tolist())) == 1
            if r + 1 < len(plan) and plan[r + 1, 0] == plan[r, 0] and k and w[-1] == words[plan[r + 1, 2] + stride]:
                straddles += 1  # the row's last word goes on behind the overlap, in the next row
        for flags in (15, 15 | T.LABELS_SHIFT, T.LABELS_TEMPLATE | T.LABELS_END | T.LABELS_SHIFT):
            check_labels(ids_t, mask_t, plan_t, flags)
    assert straddles > 10


@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("n_sep", [0, 1, 4])
def test_pairs(n_sep, dtype):
    """The three strategies; B's words begin at 0 again and are drawn apart from A's; either side alone and both; the word
    ids of the two sides in two arrays and in one."""
    import hutoken_amd
    rng = np.random.default_rng(13 + n_sep)
    L = 24
    tpl = dict(bos_id=50256, sep_ids=tuple(50250 + i for i in range(n_sep)), eos_id=50255, pad_id=7)
    R = L - 2 - n_sep
    lens = [(R // 2, R - R // 2), (R, R), (0, 2 * R), (2 * R, 0), (0, 0), (R + 3, 1), (1, R + 3), (R, 0), (0, R)]
    lens += [tuple(x) for x in rng.integers(0, L, size=(291, 2))]
    a, oa = ragged([x for x, _ in lens], rng, base=3)
    b, ob = ragged([y for _, y in lens], rng)
    wa, wb = words_of(oa, rng, len(a)), words_of(ob, rng)
    both = np.concatenate([a, b])  # one encode call: B's offsets a view with a non-zero base
    ob1 = ob + len(a)
    w1 = np.concatenate([wa, wb])
    for strategy, side in (("longest_first", "right"), ("only_first", "left"), ("only_second", "right")):
        res = hutoken_amd.collate_pairs(dev(a), dev(oa), dev(b), dev(ob), L, truncation=strategy, padding_side=side, dtype=dtype,
                                        return_plan=True, check=True, **tpl)
        ids_t, mask_t, plan_t = res[0], res[1], res[4]
        for sides in ("a", "b", "both"):
            check_mlm(ids_t, plan_t, seed=31, p=0.4, sides=sides)
            _out, labels = check_mlm(ids_t, plan_t, seed=32, p=0.5, words=wa, words_b=wb, sides=sides)
            plan = host(plan_t)
            rows = np.arange(len(plan))
            if sides == "a":  # nothing of B, of the separators or of the template carries a label
                keep = np.ones_like(labels, dtype=bool)
                for r in rows:
                    keep[r, plan[r, 4]:plan[r, 4] + plan[r, 3]] = False
                assert (labels[keep] == -100).all()
        res1 = hutoken_amd.collate_pairs(dev(both), dev(oa), dev(both), dev(ob1), L, truncation=strategy, padding_side=side, dtype=dtype,
                                         return_plan=True, check=True, **tpl)
        assert same(host(res1[0]), host(ids_t))
        got = check_mlm(res1[0], res1[4], seed=32, p=0.5, words=w1)
        two = check_mlm(ids_t, plan_t, seed=32, p=0.5, words=wa, words_b=wb)
        assert same(got[0], two[0]) and same(got[1], two[1])
        for flags in SUBSETS:
            check_labels(ids_t, mask_t, plan_t, flags)
            check_labels(ids_t, mask_t, plan_t, flags | T.LABELS_SHIFT)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_pair_windows(dtype):
    import hutoken_amd
    rng = np.random.default_rng(14)
    L, stride = 20, 3
    tpl = dict(bos_id=50256, sep_ids=(50250, 50251), eos_id=50255, pad_id=7)
    lens = [(3, 60), (0, 40), (5, 0), (16, 16), (30, 4)]  # then a short side and a long one, either way round
    lens += [(int(x), int(y)) for x, y in zip(rng.integers(0, 10, size=100), rng.integers(0, 60, size=100))]
    lens += [(int(y), int(x)) for x, y in zip(rng.integers(0, 10, size=100), rng.integers(0, 60, size=100))]
    a, oa = ragged([x for x, _ in lens], rng)
    b, ob = ragged([y for _, y in lens], rng, base=2)
    wa, wb = words_of(oa, rng), words_of(ob, rng, len(b))
    for strategy in ("only_second", "only_first"):
        res = hutoken_amd.collate_pair_windows(dev(a), dev(oa), dev(b), dev(ob), L, stride, truncation=strategy, dtype=dtype,
                                               return_plan=True, check=True, **tpl)
        ids_t, mask_t, plan_t = res[0], res[1], res[5]
        assert plan_t.shape[0] > 256
        for sides in ("a", "b", "both"):
            check_mlm(ids_t, plan_t, seed=41, p=0.5, words=wa, words_b=wb, sides=sides)
        check_mlm(ids_t, plan_t, seed=42)
        for flags in (15, 10, 10 | T.LABELS_SHIFT, 5 | T.LABELS_SHIFT):
            check_labels(ids_t, mask_t, plan_t, flags)


# ---- rules ------------------------------------------------------------------------------------------------------------
def rule_rows(dtype, L=32, n=300):
    rng = np.random.default_rng(15)
    (ids_t, mask_t, _lengths, plan_t), ids, offs = padded(list(rng.integers(0, L + 9, size=n)), L, dtype, rng, bos_id=50256, eos_id=50255, pad_id=7)
    return ids_t, mask_t, plan_t, offs, words_of(offs, rng)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_probabilities_and_fractions(dtype):
    ids_t, _mask_t, plan_t, _offs, words = rule_rows(dtype)
    ids, plan = host(ids_t), host(plan_t)
    eligible = np.zeros_like(ids, dtype=bool)
    for r, row in enumerate(plan.tolist()):
        eligible[r, row[4]:row[4] + row[3]] = True
    for w in (None, words):
        out, labels = check_mlm(ids_t, plan_t, seed=1, p=0.0, words=w)
        assert same(out, ids) and (labels == -100).all()
        out, labels = check_mlm(ids_t, plan_t, seed=1, p=1.0, words=w, ignore=-1)
        assert ((labels != -1) == eligible).all() and same(labels[eligible], ids[eligible]) and same(out[~eligible], ids[~eligible])
        out, labels = check_mlm(ids_t, plan_t, seed=2, p=1.0, mf=1.0, rf=0.0, words=w, vocab=None)
        assert (out[eligible] == MASK_ID).all()
        out, labels = check_mlm(ids_t, plan_t, seed=2, p=1.0, mf=0.0, rf=1.0, words=w, vocab=11)
        assert (out[eligible] < 11).all() and (out[eligible] >= 0).all() and len(np.unique(out[eligible])) == 11
        out, labels = check_mlm(ids_t, plan_t, seed=2, p=1.0, mf=0.0, rf=0.0, words=w, vocab=None)
        assert same(out, ids) and same(labels[eligible], ids[eligible])
    # the defaults: 15 % of the tokens, of which 80 % / 10 % / 10 %
    out, labels = check_mlm(ids_t, plan_t, seed=3)
    sel = labels != -100
    n, k = int(eligible.sum()), int(sel.sum())
    assert abs(k - 0.15 * n) < 5 * (n * 0.15 * 0.85) ** 0.5  # five sigma of a binomial count
    masked = int((out[sel] == MASK_ID).sum())
    assert abs(masked - 0.8 * k) < 5 * (k * 0.8 * 0.2) ** 0.5


@pytest.mark.parametrize("dtype", WIDTHS)
def test_protected_words(dtype):
    ids_t, _mask_t, plan_t, _offs, words = rule_rows(dtype)
    rng = np.random.default_rng(16)
    guarded = words.copy()
    guarded[rng.random(len(words)) < 0.3] = -1
    out, labels = check_mlm(ids_t, plan_t, seed=4, p=1.0, words=guarded)
    ids, plan = host(ids_t), host(plan_t)
    for r, row in enumerate(plan.tolist()):
        w = guarded[row[2]:row[2] + row[3]]
        cols = slice(row[4], row[4] + row[3])
        assert ((labels[r, cols] != -100) == (w >= 0)).all() and same(out[r, cols][w < 0], ids[r, cols][w < 0])


@pytest.mark.parametrize("dtype", WIDTHS)
def test_a_row_depends_on_its_number_and_the_seed_alone(dtype):
    import hutoken_amd
    ids_t, _mask_t, plan_t, _offs, words = rule_rows(dtype)
    for w in (None, dev(words)):
        kw = dict(mask_id=MASK_ID, vocab_size=VOCAB, mlm_probability=0.3, word_ids=w)
        out, labels = (host(x) for x in hutoken_amd.mask_tokens(ids_t, plan_t, seed=2**64 - 1, **kw))
        again = [host(x) for x in hutoken_amd.mask_tokens(ids_t, plan_t, seed=2**64 - 1, **kw)]
        assert same(again[0], out) and same(again[1], labels)
        for k in (1, 257):  # the first k rows alone: a batch of another size, tiled in another way
            part = [host(x) for x in hutoken_amd.mask_tokens(ids_t[:k].contiguous(), plan_t[:k].contiguous(), seed=2**64 - 1, **kw)]
            assert same(part[0], out[:k]) and same(part[1], labels[:k])
        other = [host(x) for x in hutoken_amd.mask_tokens(ids_t, plan_t, seed=2**63, **kw)]
        assert not same(other[1], labels) and not same(other[0], out)
    # the two widths draw alike
    if dtype == "int64":
        import torch
        narrow = hutoken_amd.mask_tokens(ids_t.to(torch.int32), plan_t, mask_id=MASK_ID, vocab_size=VOCAB, seed=9)
        wide = hutoken_amd.mask_tokens(ids_t, plan_t, mask_id=MASK_ID, vocab_size=VOCAB, seed=9)
        assert all(same(host(a).astype(np.int64), host(b)) for a, b in zip(narrow, wide))


def test_wide_ids_and_fills_go_through_whole():
    """int64 rows whose ids and ignore index need more than 32 bits"""
    import hutoken_amd
    ids_t, mask_t, plan_t, _offs, _words = rule_rows("int64", L=8, n=40)
    big = ids_t + 2**40
    out, labels = check_mlm(big, plan_t, seed=6, p=0.5, ignore=-2**50)
    assert (labels[labels != -2**50] >= 2**40).all() and (out[(out != MASK_ID) & (labels == -2**50)] >= 2**40).all()
    want = check_labels(big, mask_t, plan_t, 15 | T.LABELS_SHIFT, ignore=2**62)
    assert (want >= 2**40).all()


# ---- labels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("side", ["right", "left"])
def test_label_flags_on_padded_rows(side, dtype):
    """Every subset of the selecting flags, with and without shift; documents that fill the row (the last real column is
    L - 1); with left padding the last pad column predicts nothing."""
    rng = np.random.default_rng(17)
    for L in (12, 7):
        lens = [L + 4, L - 2, L - 3, 0, 1] + list(rng.integers(0, L + 4, size=295))
        (ids_t, mask_t, lengths, plan_t), _ids, _offs = padded(lens, L, dtype, rng, bos_id=50256, eos_id=50255, pad_id=7, padding_side=side)
        assert host(lengths)[:3].tolist() == [L, L, L - 1]
        for flags in SUBSETS:
            check_labels(ids_t, mask_t, plan_t, flags)
            want = check_labels(ids_t, mask_t, plan_t, flags | T.LABELS_SHIFT)
            assert (want[:, L - 1] == -100).all()
            if side == "left":
                pads = L - host(lengths)
                rows = np.nonzero(pads > 0)[0]
                assert (want[rows, pads[rows] - 1] == -100).all()
        ids = host(ids_t)
        want = check_labels(ids_t, mask_t, plan_t, 15 | T.LABELS_SHIFT)
        assert same(want[0, :L - 1], ids[0, 1:])  # the full row predicts every column but its first


@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [4097, 8195, 8192])
def test_labels_across_the_column_chunks(L, dtype):
    """A workgroup holds 4096 columns of a long row: column 4095 predicts column 4096, which another workgroup holds."""
    rng = np.random.default_rng(L)
    for side in ("right", "left"):
        (ids_t, mask_t, _lengths, plan_t), _ids, _offs = padded([L + 5, 4095, 4097, 0], L, dtype, rng, bos_id=50256, eos_id=50255, pad_id=7,
                                                               padding_side=side)
        ids = host(ids_t)
        for flags in (15, T.LABELS_A, T.LABELS_END, T.LABELS_TEMPLATE | T.LABELS_B):
            want = check_labels(ids_t, mask_t, plan_t, flags | T.LABELS_SHIFT)
            check_labels(ids_t, mask_t, plan_t, flags)
        want = check_labels(ids_t, mask_t, plan_t, 15 | T.LABELS_SHIFT)
        assert want[0, 4095] == ids[0, 4096] and want[0, 4094] == ids[0, 4095]
        if L > 8192:
            assert want[0, 8191] == ids[0, 8192]


def init(preset="gpt2"):
    import hutoken_amd
    from hutoken_amd import data
    vp, sp, _kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, is_byte_encoder=True, pretokenizer=preset)
    return hutoken_amd


def test_completion_labels_on_encoded_pairs():
    hutoken = init()
    tpl = dict(bos_id=50256, sep_ids=(50255,), eos_id=50254, pad_id=-9)
    for L, side in ((24, "right"), (16, "left")):
        ids_t, mask_t, types_t, lengths_t, plan_t = hutoken.batch_encode_pairs(FC.QUESTIONS, FC.CONTEXTS, L, padding_side=side, return_plan=True, **tpl)
        for shift in (False, True):
            got = host(hutoken.lm_labels(ids_t, mask_t, plan_t, loss_on="completion", shift=shift, check=True))
            want, wrong = T.labels_ref(host(ids_t), host(mask_t), host(plan_t), T.LABELS_B | T.LABELS_END | (T.LABELS_SHIFT if shift else 0))
            assert not wrong and same(got, want)
        ids, plan, got = host(ids_t), host(plan_t), host(hutoken.lm_labels(ids_t, mask_t, plan_t, loss_on="completion"))
        for r, row in enumerate(plan.tolist()):  # the answer and eos carry loss; the question, bos, the separator and padding none
            end = row[7] + row[6]
            assert same(got[r, row[7]:end + 1], ids[r, row[7]:end + 1]) and got[r, end] == 50254
            assert (got[r, :row[7]] == -100).all() and (got[r, end + 1:] == -100).all()
        assert same(host(hutoken.lm_labels(ids_t, mask_t, plan_t)), np.where(host(mask_t) != 0, ids, -100).astype(ids.dtype))


# ---- hostile plans ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [8, 7, 4100])
def test_hostile_plans_stay_inside_their_buffers(L, dtype):
    """A plan is a caller's tensor.  Whatever it holds, nothing is read outside the word ids or written outside the two
    outputs: HUTK_E_ARG, a guard band left as it was, and every row as the restatement has it."""
    import torch
    import hutoken_amd
    rng = np.random.default_rng(18)
    n_w = 40
    words = rng.integers(0, 6, size=n_w).astype(np.int32)
    big = 2**62
    whole = min(L, n_w)
    sound = [[0, 0, 3, 4, 1, 2, 2, 5], [1, 0, 0, 0, 0, 0, 0, 0], [2, 0, n_w - whole, whole, 0, 0, 0, whole]]
    defects = {"src_a behind the words": [0, 0, n_w - 2, 4, 0, 0, 0, 4],
               "src_a negative": [0, 0, -3, 4, 0, 0, 0, 4],
               "src_b far away": [0, 0, 0, 2, 0, big, 3, 3],
               "src_a at the lowest value": [0, 0, -2**63, 2, 0, 0, 0, 2],
               "ka negative": [0, 0, 0, -5, 0, 1, 2, 3],
               "kb negative": [0, 0, 0, 2, 0, 1, -big, 3],
               "col_a beyond the row": [0, 0, 0, 3, L + 3, 0, 0, L + 6],
               "col_a at the row's end": [0, 0, 0, 1, L, 0, 0, L + 1],
               "col_b negative": [0, 0, 0, 2, 0, 4, 3, -2],
               "col_a far away": [0, 0, 0, 3, big, 0, 3, -big],
               "ka leaves the row": [0, 0, 0, L + 1, 0, 0, 0, L + 1],
               "ka huge": [0, 0, 0, 2**63 - 1, 2, 0, 2**63 - 1, 2**63 - 1],
               "kb leaves the row": [0, 0, 0, 2, 0, 0, L, 2],
               "sides overlap": [0, 0, 0, 4, 1, 5, 3, 3]}
    only_words = ("src_a behind the words", "src_a negative", "src_b far away", "src_a at the lowest value")
    tdt = getattr(torch, dtype)
    width = 4 if dtype == "int32" else 8
    guard = 64
    for name, rows in [("sound", sound)] + [(k, [v]) for k, v in defects.items()] + [("all", sound + list(defects.values()))]:
        plan = np.array(rows, dtype=np.int64)
        n = len(plan)
        ids = rng.integers(100, 50000, size=(n, L)).astype(dtype)
        mask = (rng.random((n, L)) < 0.8).astype(np.uint8)
        d_plan, d_ids, d_mask = dev(plan), dev(ids), dev(mask)
        for w in (None, words):
            want = T.mlm_ref(ids, plan, w, seed=5, mask_id=MASK_ID, vocab_size=VOCAB, **thresholds(0.5, 0.8, 0.1))
            assert want[2] == (name != "sound" and (w is not None or name not in only_words)), name
            s_out = torch.full((guard + n * L + guard,), 77, dtype=tdt, device="cuda:0")
            s_lab = torch.full((guard + n * L + guard,), 77, dtype=tdt, device="cuda:0")
            rc = raw_mlm(d_plan, d_ids, s_out[guard:guard + n * L], s_lab[guard:guard + n * L], L, width, None if w is None else dev(w))
            assert rc == (E_ARG if want[2] else 0), (L, name, rc)
            for store, rect in ((s_out, want[0]), (s_lab, want[1])):
                got = host(store)
                assert (got[:guard] == 77).all() and (got[guard + n * L:] == 77).all(), (L, name)
                assert same(got[guard:guard + n * L].reshape(n, L), rect), (L, name)
            call = lambda: hutoken_amd.mask_tokens(d_ids, d_plan, mask_id=MASK_ID, vocab_size=VOCAB, seed=5, mlm_probability=0.5,  # noqa: E731
                                                   word_ids=None if w is None else dev(w), check=True)
            if want[2]:
                with pytest.raises(ValueError, match="row_plan"):
                    call()
            else:
                assert same(host(call()[0]), want[0])
        for flags in (15, 15 | T.LABELS_SHIFT, T.LABELS_B | T.LABELS_TEMPLATE | T.LABELS_SHIFT):
            want, wrong = T.labels_ref(ids, mask, plan, flags)
            assert wrong == (name != "sound" and name not in only_words), name
            s_lab = torch.full((guard + n * L + guard,), 77, dtype=tdt, device="cuda:0")
            rc = raw_labels(d_plan, d_ids, d_mask, s_lab[guard:guard + n * L], L, width, flags)
            assert rc == (E_ARG if wrong else 0), (L, name, rc)
            got = host(s_lab)
            assert (got[:guard] == 77).all() and (got[guard + n * L:] == 77).all(), (L, name)
            assert same(got[guard:guard + n * L].reshape(n, L), want), (L, name, flags)
        if name == "all":
            with pytest.raises(ValueError, match="row_plan"):
                hutoken_amd.lm_labels(d_ids, d_mask, d_plan, check=True)


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_batch_encode_mlm():
    hutoken = init()
    texts = FC.NER_TEXTS + FC.CONTEXTS + FC.short_texts(30)
    kw = dict(bos_id=50256, eos_id=50255, pad_id=50254)
    for L, side in ((24, "right"), (None, "left")):
        plain = hutoken.batch_encode_padded(texts, L, padding_side=side, return_word_ids=True, **kw)
        ids, word_ids = host(plain[0]), host(plain[3])
        for whole_word in (False, True):
            res = hutoken.batch_encode_mlm(texts, L, mask_id=MASK_ID, seed=77, vocab_size=VOCAB, whole_word=whole_word, mlm_probability=0.3,
                                           padding_side=side, **kw)
            assert len(res) == 4
            out, mask, lengths, labels = (host(x) for x in res)
            assert same(mask, host(plain[1])) and same(lengths, host(plain[2])) and out.shape == ids.shape
            sel = labels != -100
            assert same(np.where(sel, labels, out), ids)  # the labels put back give the rows as they were
            assert sel.any() and not sel[word_ids < 0].any() and (out != ids).any() and not (out != ids)[~sel].any()
            if whole_word:
                for r in range(len(ids)):
                    for word in np.unique(word_ids[r][word_ids[r] >= 0]):
                        assert len(set(sel[r][word_ids[r] == word].tolist())) == 1, (r, word)
                assert any(int((word_ids[r] == w).sum()) > 1 and sel[r][word_ids[r] == w].all()
                           for r in range(len(ids)) for w in np.unique(word_ids[r][word_ids[r] >= 0]))
            again = hutoken.batch_encode_mlm(texts, L, mask_id=MASK_ID, seed=77, vocab_size=VOCAB, whole_word=whole_word, mlm_probability=0.3,
                                             padding_side=side, **kw)
            assert same(host(again[0]), out) and same(host(again[3]), labels)
    hutoken.set_pretokenizer(None)  # the built-in splitter: whole words are refused before anything is encoded
    with pytest.raises(ValueError, match="split preset"):
        hutoken.batch_encode_mlm(texts, 24, mask_id=MASK_ID, seed=1, vocab_size=VOCAB, whole_word=True)
    res = hutoken.batch_encode_mlm(texts[:3], 16, mask_id=MASK_ID, seed=1, vocab_size=VOCAB)  # token mode needs no preset
    assert len(res) == 4 and res[3].shape == (3, 16)


def test_on_the_default_and_on_a_non_default_stream():
    import torch
    import hutoken_amd
    ids_t, mask_t, plan_t, _offs, words = rule_rows("int32")
    w = dev(words)

    def run():
        a = hutoken_amd.mask_tokens(ids_t, plan_t, mask_id=MASK_ID, vocab_size=VOCAB, seed=8, word_ids=w)
        return a + (hutoken_amd.lm_labels(a[0], mask_t, plan_t, loss_on="completion", shift=True), hutoken_amd.lm_labels(ids_t, mask_t, plan_t))
    assert torch.cuda.current_stream().cuda_stream == 0
    on_default = [host(x) for x in run()]
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        on_side = run()
        torch.cuda.synchronize()
    assert all(same(a, host(b)) for a, b in zip(on_default, on_side))
    want = T.mlm_ref(host(ids_t), host(plan_t), words, seed=8, mask_id=MASK_ID, vocab_size=VOCAB, **thresholds(0.15, 0.8, 0.1))
    assert same(on_default[0], want[0]) and same(on_default[1], want[1])
