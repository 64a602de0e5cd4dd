"""Pair collation on the GPU (csrc/hutk_collate.hip: k_pair_count, k_pair_write, k_collate_pairs) against the NumPy
reference of tests/pairs_ref.py, every comparison exact and over every element of every output.

The reference's row table (every row's pair, window start, ka and kb) is expanded to the rectangle on the device by
torch_rows below; up to NUMPY_MAX output elements the result is also compared with the reference's vectorised form, and
for small batches with its loop form (which tests/test_pairs_cpu.py pins by hand and against `tokenizers`).  Needs a
real MI355X."""
import itertools
import unicodedata

import numpy as np
import pytest

import pairs_ref as R

pytestmark = pytest.mark.gpu

TEMPLATES = [{}, {"sep_ids": (4,), "eos_id": 50256}, {"bos_id": -5, "sep_ids": (4, -6), "eos_id": 50256},
             {"bos_id": 1, "sep_ids": ()}]
COMBOS = [(np.int32, "right"), (np.int64, "left"), (np.int32, "left"), (np.int64, "right")]
NUMPY_MAX = 1 << 19
LOOP_MAX = 3000  # ids, pairs and rows
PAD = -9


def n_special(kw):
    return ("bos_id" in kw) + len(kw.get("sep_ids", ())) + ("eos_id" in kw)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def tdtype(dtype):
    import torch
    return torch.int64 if dtype == np.int64 else torch.int32


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def torch_rows(d_a, oa, d_b, ob, table, L, side, dtype, bos_id=None, sep_ids=(), eos_id=None):
    """pairs_ref.expand on the device: table = (pair, start_a, start_b, ka, kb), NumPy int64 arrays of one entry per row."""
    import torch
    pair, sa, sb, ka, kb = (dev(np.asarray(x, dtype=np.int64)) for x in table)
    d_oa, d_ob = dev(np.asarray(oa, dtype=np.int64)), dev(np.asarray(ob, dtype=np.int64))
    has_bos, n_sep = int(bos_id is not None), len(sep_ids)
    s = has_bos + n_sep + (eos_id is not None)
    c = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda:0")  # noqa: E731
    sl = ka + kb + s
    shift = L - sl if side == "left" else torch.zeros_like(sl)
    q = torch.arange(L, device="cuda:0")[None, :] - shift[:, None]
    valid = (q >= 0) & (q < sl[:, None])
    end_a = (has_bos + ka)[:, None]
    end_sep = end_a + n_sep
    in_a = valid & (q >= has_bos) & (q < end_a)
    in_b = valid & (q >= end_sep) & (q < end_sep + kb[:, None])
    src_a = torch.cat([d_a, torch.zeros(1, dtype=torch.int32, device="cuda:0")])
    src_b = torch.cat([d_b, torch.zeros(1, dtype=torch.int32, device="cuda:0")])
    out = torch.where(in_a, src_a[((d_oa[pair] + sa)[:, None] + q - has_bos).clamp_(0, src_a.numel() - 1)], c(PAD))
    out = torch.where(in_b, src_b[((d_ob[pair] + sb)[:, None] + q - end_sep).clamp_(0, src_b.numel() - 1)], out)
    del in_a, in_b
    if has_bos:
        out = torch.where(valid & (q == 0), c(bos_id), out)
    for u, t in enumerate(sep_ids):
        out = torch.where(valid & (q == end_a + u), c(t), out)
    if eos_id is not None:
        out = torch.where(q == sl[:, None] - 1, c(eos_id), out)
    return out.to(tdtype(dtype)), valid.to(torch.uint8), (valid & (q >= end_sep)).to(torch.uint8), sl.to(torch.int32)


def one_row_table(oa, ob, L, strategy, kw):
    ka, kb = R.pair_lengths_vec(np.diff(oa), np.diff(ob), L - n_special(kw), strategy)
    zero = np.zeros(len(oa) - 1, dtype=np.int64)
    return np.arange(len(oa) - 1, dtype=np.int64), zero, zero, ka, kb


def window_table(oa, ob, L, stride, strategy, kw):
    _ro, pair, start, ka, kb = R.row_table(oa, ob, L, stride, strategy, **kw)
    zero = np.zeros_like(start)
    return (pair, zero, start, ka, kb) if strategy == "only_second" else (pair, start, zero, ka, kb)


def compare(got, want, label):
    import torch
    assert len(got) == len(want), label
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), label


def check(a, oa, b, ob, L, strategy, dtype=np.int32, side="right", label=None, d=None, **kw):
    """One collate_pairs call against the reference: all four outputs, every element.  d: the inputs already on the
    device (d_a, d_oa, d_b, d_ob).  -> the device tensors."""
    import hutoken_amd
    d_a, d_oa, d_b, d_ob = d or (dev(a), dev(oa), dev(b), dev(ob))
    got = hutoken_amd.collate_pairs(d_a, d_oa, d_b, d_ob, L, truncation=strategy, dtype=tdtype(dtype), pad_id=PAD,
                                    padding_side=side, check=True, **kw)
    label = (label, L, strategy, kw, dtype, side)
    compare(got, torch_rows(d_a, oa, d_b, ob, one_row_table(oa, ob, L, strategy, kw), L, side, dtype, **kw), label)
    if got[0].numel() <= NUMPY_MAX:
        host = [g.cpu().numpy() for g in got]
        args = (a, oa, b, ob, L, strategy)
        assert all(same(g, w) for g, w in zip(host, R.pairs_vec(*args, pad_id=PAD, padding_side=side, dtype=dtype, **kw))), label
        if len(a) + len(b) <= LOOP_MAX and len(oa) <= LOOP_MAX:
            assert all(same(g, w) for g, w in zip(host, R.pairs(*args, pad_id=PAD, padding_side=side, dtype=dtype, **kw))), label
    return got


def check_windows(a, oa, b, ob, L, stride, strategy, dtype=np.int32, side="right", label=None, d=None, n_rows=None, **kw):
    """One collate_pair_windows call against the reference: all five outputs, every element.  -> the device tensors."""
    import torch
    import hutoken_amd
    d_a, d_oa, d_b, d_ob = d or (dev(a), dev(oa), dev(b), dev(ob))
    got = hutoken_amd.collate_pair_windows(d_a, d_oa, d_b, d_ob, L, stride, truncation=strategy, dtype=tdtype(dtype),
                                           pad_id=PAD, padding_side=side, check=True, n_rows=n_rows, **kw)
    label = (label, L, stride, strategy, kw, dtype, side)
    table = window_table(oa, ob, L, stride, strategy, kw)
    want = torch_rows(d_a, oa, d_b, ob, table, L, side, dtype, **kw)
    start = table[2] if strategy == "only_second" else table[1]
    compare(got, want + (torch.stack([dev(table[0]), dev(start)], dim=1),), label)
    if got[0].numel() <= NUMPY_MAX:
        host = [g.cpu().numpy() for g in got]
        args = (a, oa, b, ob, L, stride, strategy)
        assert all(same(g, w) for g, w in zip(host, R.pair_windows_vec(*args, pad_id=PAD, padding_side=side, dtype=dtype, **kw))), label
        if len(a) + len(b) <= LOOP_MAX and len(oa) <= LOOP_MAX and len(host[0]) <= LOOP_MAX:
            assert all(same(g, w) for g, w in zip(host, R.pair_windows(*args, pad_id=PAD, padding_side=side, dtype=dtype, **kw))), label
    return got


def ragged_from(lens, rng, base=0, tail=0):
    """lengths -> (ids int32 with negative ones among them, offsets int64 that begin at `base`)"""
    offs = np.full(len(lens) + 1, base, dtype=np.int64)
    offs[1:] += np.cumsum(lens, dtype=np.int64)
    return rng.integers(-3, 60000, size=int(offs[-1]) + tail).astype(np.int32), offs


def random_lens(rng, n, L):
    """mostly short documents, one in eight up to 1.2 L ids: pairs that fit, pairs where one side is cut, and both"""
    lens = rng.integers(0, 41, size=n)
    long = rng.random(n) < 0.125
    return np.where(long, rng.integers(0, L + L // 5 + 2, size=n), lens)


def combos_for(i, elements):
    """every (dtype, side) for small outputs; one of them, in turn, for large ones (which path a dtype and a side take
    does not depend on the size)"""
    return COMBOS if elements <= NUMPY_MAX else [COMBOS[i % 4]]


@pytest.mark.parametrize("L", ["s+1", 7, 8, 64, 100, 2048, 5000])  # 5000: column chunks; 7 and 100: element stores
@pytest.mark.parametrize("n_pairs", [0, 1, 2, 63, 64, 65, 257, 5000])
def test_random_ragged_batches(n_pairs, L):
    rng = np.random.default_rng(1000 * n_pairs + (3 if L == "s+1" else L))
    Lmax = 12 if L == "s+1" else L
    a, oa = ragged_from(random_lens(rng, n_pairs, Lmax), rng, base=int(rng.integers(0, 4)), tail=2)
    b, ob = ragged_from(random_lens(rng, n_pairs, Lmax), rng, base=int(rng.integers(0, 9)))
    d = (dev(a), dev(oa), dev(b), dev(ob))
    for i, (kw, strategy) in enumerate(itertools.product(TEMPLATES, R.STRATEGIES)):
        Lk = n_special(kw) + 1 if L == "s+1" else L
        if Lk < n_special(kw) + 1:
            continue
        for dtype, side in combos_for(i, n_pairs * Lk):
            check(a, oa, b, ob, Lk, strategy, dtype, side, label=n_pairs, d=d, **kw)


def edge_lengths(Rm):
    return sorted({n for n in (0, 1, Rm // 2 - 1, Rm // 2, Rm // 2 + 1, Rm - 1, Rm, Rm + 1, 3 * Rm) if n >= 0})


@pytest.mark.parametrize("Rm", [1, 2, 5, 8, 63, 64])  # R odd and even; 8 and 64 with an even s: the 16-byte stores
def test_lengths_on_every_edge_of_the_formulas(Rm):
    rng = np.random.default_rng(Rm)
    crossed = list(itertools.product(edge_lengths(Rm), repeat=2))
    a, oa = ragged_from([na for na, _ in crossed], rng)
    b, ob = ragged_from([nb for _, nb in crossed], rng, base=5)
    d = (dev(a), dev(oa), dev(b), dev(ob))
    for i, (kw, strategy) in enumerate(itertools.product(TEMPLATES, R.STRATEGIES)):
        L = Rm + n_special(kw)
        for dtype, side in COMBOS:  # as neighbours in one batch
            got = check(a, oa, b, ob, L, strategy, dtype, side, label="batch", d=d, **kw)
        lengths = got[3].cpu().numpy()
        for j, (na, nb) in enumerate(crossed):
            assert lengths[j] == min(na + nb, Rm) + n_special(kw)
        if kw is not TEMPLATES[2]:
            continue
        dtype, side = COMBOS[i % 4]
        for j, (na, nb) in enumerate(crossed):  # ... and each pair alone, through views of the batch's tensors
            one = (d[0], d[1][j:j + 2], d[2], d[3][j:j + 2])
            check(a, oa[j:j + 2], b, ob[j:j + 2], L, strategy, dtype, side, label=(na, nb), d=one, **kw)


def window_edge_lengths(C, step):
    return sorted({n for n in (0, 1, C - 1, C, C + 1, C + step - 1, C + step, C + step + 1, C + 5 * step) if n >= 0})


# (R, ids of the kept side, stride): C = R - min(kept, R), step = max(1, C - stride)
WINDOW_EDGES = [(1, 0, 0), (2, 0, 1), (2, 0, 0), (5, 0, 4), (5, 2, 1), (7, 2, 3), (64, 0, 63), (64, 31, 0), (64, 10, 20),
                (5, 5, 2), (5, 9, 2),    # C == 0: one row, the cut side empty (the kept side itself cut in the second)
                (8, 6, 4), (8, 7, 1), (8, 5, 3)]  # C <= stride: the step is 1


@pytest.mark.parametrize("Rm,kept,stride", WINDOW_EDGES)
def test_windows_on_every_edge_of_the_formula(Rm, kept, stride):
    rng = np.random.default_rng(Rm * 1000 + kept * 10 + stride)
    _ko, C, step = R.window_sizes(kept, Rm, stride)
    lens = window_edge_lengths(C, step)
    order = lens + lens[::-1]
    cut, oc = ragged_from(order, rng, base=3)
    other, oo = ragged_from([kept] * len(order), rng)
    for strategy in ("only_first", "only_second"):
        a, oa, b, ob = (other, oo, cut, oc) if strategy == "only_second" else (cut, oc, other, oo)
        d = (dev(a), dev(oa), dev(b), dev(ob))
        for i, kw in enumerate(TEMPLATES):
            L = Rm + n_special(kw)
            for dtype, side in COMBOS:  # as neighbours in one batch
                got = check_windows(a, oa, b, ob, L, stride, strategy, dtype, side, label="batch", d=d, **kw)
            assert got[0].shape[0] == sum(R.window_count(n, kept, Rm, stride) for n in order)
            if C == 0:
                assert got[0].shape[0] == len(order)
            dtype, side = COMBOS[i % 4]
            for j, n in enumerate(order[:len(lens)]):  # ... and each pair alone
                one = (d[0], d[1][j:j + 2], d[2], d[3][j:j + 2])
                got = check_windows(a, oa[j:j + 2], b, ob[j:j + 2], L, stride, strategy, dtype, side, label=n, d=one, **kw)
                assert got[0].shape[0] == R.window_count(n, kept, Rm, stride)


@pytest.mark.parametrize("L", [7, 16, 64, 5000])
def test_windows_of_mixed_pairs(L):
    """Short and long kept sides side by side, so that C differs from row to row inside one workgroup (C == 0 and
    C <= stride among them), and cut sides long enough that workgroup boundaries fall inside one pair's windows."""
    rng = np.random.default_rng(L)
    n = 300 if L < 5000 else 40
    for i, kw in enumerate(TEMPLATES):
        Rm = L - n_special(kw)
        kept = rng.integers(0, Rm + 3, size=n)
        kept[rng.random(n) < 0.3] = 0
        kept[n // 2] = Rm // 2
        other, oo = ragged_from(kept, rng, base=2)
        C = Rm - np.minimum(kept, Rm)
        for stride in sorted({0, 1, Rm // 2, Rm - 1}):
            step = np.maximum(1, C - stride)
            windows = np.where(rng.random(n) < 0.3, rng.integers(0, 31, size=n), 0)  # at most 31 rows a pair ...
            cut_lens = np.where(windows > 0, C + step * windows - rng.integers(0, step), rng.integers(0, Rm + 2, size=n))
            if L < 5000:
                cut_lens[n // 2] = C[n // 2] + step[n // 2] * 3000  # ... but for one that lies over several workgroups
            cut, oc = ragged_from(np.maximum(cut_lens, 0), rng, base=1)
            for strategy in ("only_first", "only_second"):
                a, oa, b, ob = (other, oo, cut, oc) if strategy == "only_second" else (cut, oc, other, oo)
                dtype, side = COMBOS[(i + stride) % 4]
                got = check_windows(a, oa, b, ob, L, stride, strategy, dtype, side, label="mixed", **kw)
                assert got[0].shape[0] >= (3000 if L < 5000 else n)


def test_one_pair_over_many_workgroups_and_many_pairs_in_one():
    rng = np.random.default_rng(3)
    cut, oc = ragged_from([100_000], rng)
    other, oo = ragged_from([2], rng)
    for i, (dtype, side) in enumerate(COMBOS):
        got = check_windows(other, oo, cut, oc, 7, 2, "only_second", dtype, side, bos_id=1)  # C = 4, step 2: element stores
        assert got[0].shape == (49_999, 7)
    got = check_windows(cut, oc, other, oo, 8, 4, "only_first")  # C = 6, step 2: the 16-byte path
    assert got[0].shape == (49_998, 8)
    for lens in ([0] * 50_000 + [10_000], [10_000] + [0] * 50_000):  # a search that ends among thousands of one-row pairs
        cut, oc = ragged_from(lens, rng)
        other, oo = ragged_from([1] * len(lens), rng)
        check_windows(other, oo, cut, oc, 16, 3, "only_second", np.int32, "right", sep_ids=(4,))
        check_windows(cut, oc, other, oo, 7, 3, "only_first", np.int64, "left", eos_id=2)


def test_the_scan_across_blocks():
    """300 000 pairs: more than one chunk of the scan over the workgroup sums."""
    import torch
    from hutoken_amd import _capi
    n, L, stride = 300_000, 16, 3
    rng = np.random.default_rng(8)
    a, oa = ragged_from(rng.integers(0, 12, size=n), rng, base=7)
    b, ob = ragged_from(rng.integers(0, 41, size=n), rng)
    kw = TEMPLATES[1]
    want_ro = R.row_table(oa, ob, L, stride, "only_second", **kw)[0]
    d = (dev(a), dev(oa), dev(b), dev(ob))
    d_ro = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    err = torch.ones(1, dtype=torch.int32, device="cuda:0")
    _capi.pair_rows_device(d[1].data_ptr(), d[3].data_ptr(), n, len(a), len(b), L, stride, _capi.PAIR_ONLY_SECOND,
                           _capi.NO_TOKEN, kw["sep_ids"], kw["eos_id"], d_ro.data_ptr(), err.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    assert int(err.item()) == 0
    assert np.array_equal(d_ro.cpu().numpy(), want_ro)
    got = check_windows(a, oa, b, ob, L, stride, "only_second", d=d, **kw)
    host = [g.cpu().numpy() for g in got]
    for p in sorted({p + e for p in list(range(0, n, 256)) + [n - 1] for e in (-1, 0, 1) if 0 <= p + e < n})[:600]:
        r0, r1 = int(want_ro[p]), int(want_ro[p + 1])  # the rows of the pairs on both sides of a boundary, by the loop form
        want = R.pair_windows(a, oa[p:p + 2], b, ob[p:p + 2], L, stride, "only_second", pad_id=PAD, **kw)
        want[4][:, 0] = p
        assert all(same(g[r0:r1], w) for g, w in zip(host, want)), p


def test_n_rows_given_right_and_wrong():
    import hutoken_amd
    rng = np.random.default_rng(31)
    a, oa = ragged_from(rng.integers(0, 9, size=100), rng)
    b, ob = ragged_from(rng.integers(0, 60, size=100), rng, base=4)
    d = (dev(a), dev(oa), dev(b), dev(ob))
    kw = dict(bos_id=1, sep_ids=(4,), eos_id=2)
    good = check_windows(a, oa, b, ob, 16, 3, "only_second", d=d, **kw)
    n_rows = good[0].shape[0]
    assert n_rows == int(R.row_table(oa, ob, 16, 3, "only_second", **kw)[0][-1]) > 100
    again = check_windows(a, oa, b, ob, 16, 3, "only_second", d=d, n_rows=n_rows, **kw)  # no synchronising read
    assert all(same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(again, good))
    for off_by in (-1, 1):  # inside the bound and wrong: the kernel finds row_offsets[-1] != n_rows
        with pytest.raises(ValueError, match="device-side error 4"):
            hutoken_amd.collate_pair_windows(*d, 16, 3, n_rows=n_rows + off_by, check=True, **kw)
    for bad in (99, 100 + len(b) + 1):  # outside [n_pairs, bound]: refused before anything is allocated
        with pytest.raises(ValueError, match="n_rows must be in"):
            hutoken_amd.collate_pair_windows(*d, 16, 3, n_rows=bad, **kw)


# ---- views, guards and bad offsets through the C ABI ------------------------------------------------------------------
GUARD = 64
FILL = {"out": -12345, "mask": 0xEE, "types": 0xEE, "lengths": -12345, "row_map": -12345}


def guarded(n, dtype, shift, fill):
    import torch
    buf = torch.full((shift + n + GUARD,), fill, dtype=dtype, device="cuda:0")
    return buf, buf[shift:shift + n]


def guards_untouched(buf, view, fill):
    lead = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lead] == fill).all()) and bool((buf[lead + view.numel():] == fill).all())


def raw_pairs(d, L, stride, strategy, kw, flags, dtype, shift, windows, expect_err=0):
    """The C ABI on output views that begin `shift` elements into buffers with guard elements on both sides.
    -> the outputs (row_offsets first in the windows form); asserts the guards and the error words."""
    import torch
    from hutoken_amd import _capi
    d_a, d_oa, d_b, d_ob = d
    n = d_oa.numel() - 1
    st = torch.cuda.current_stream().cuda_stream
    bos, sep, eos = kw.get("bos_id", _capi.NO_TOKEN), kw.get("sep_ids", ()), kw.get("eos_id", _capi.NO_TOKEN)
    err = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    n_rows, ro, ro_buf = n, None, None
    if windows:
        ro_buf, ro = guarded(n + 1, torch.int64, shift, -12345)
        _capi.pair_rows_device(d_oa.data_ptr(), d_ob.data_ptr(), n, d_a.numel(), d_b.numel(), L, stride, strategy, bos, sep,
                               eos, ro.data_ptr(), err.data_ptr(), st)
        host_ro = ro.cpu().numpy()
        assert host_ro[0] == 0 and (np.diff(host_ro) >= 1).all()  # always written, always strictly increasing
        assert guards_untouched(ro_buf, ro, -12345)
        n_rows = int(host_ro[-1])
    bufs = {"out": guarded(n_rows * L, dtype, shift, FILL["out"]), "mask": guarded(n_rows * L, torch.uint8, shift, FILL["mask"]),
            "types": guarded(n_rows * L, torch.uint8, shift, FILL["types"]),
            "lengths": guarded(n_rows, torch.int32, shift, FILL["lengths"]),
            "row_map": guarded(2 * n_rows, torch.int64, shift, FILL["row_map"])}
    v = {k: x[1] for k, x in bufs.items()}
    _capi.collate_pairs_device(d_a.data_ptr(), d_oa.data_ptr(), d_b.data_ptr(), d_ob.data_ptr(), ro.data_ptr() if windows else 0,
                               n, d_a.numel(), d_b.numel(), n_rows, L, stride, strategy, bos, sep, eos, PAD, flags,
                               dtype.itemsize, v["out"].data_ptr(), v["mask"].data_ptr(), v["types"].data_ptr(),
                               v["lengths"].data_ptr(), v["row_map"].data_ptr(), err[1:].data_ptr(), st)
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert guards_untouched(buf, view, FILL[k]), k
    assert err.tolist() == [expect_err if windows else 0, expect_err]
    res = (v["out"].view(n_rows, L), v["mask"].view(n_rows, L), v["types"].view(n_rows, L), v["lengths"], v["row_map"].view(n_rows, 2))
    return ((ro,) + res) if windows else res


def test_shared_ids_from_one_encode_call(vg_files):
    """ids_a is ids_b, offsets_b = oo[n:]: a view with a non-zero base that is off the 16-byte boundary for odd n."""
    import torch
    import hutoken_amd
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    rng = np.random.default_rng(6)
    words = ["pair", " query", " the", " passage", " 12345", "\n", " tokens", " a", " reranker", "é"]
    n = 65
    texts = ["".join(words[i] for i in rng.integers(0, len(words), size=k))
             for k in list(rng.integers(0, 12, size=n)) + list(rng.integers(0, 200, size=n))]
    raw = [t.encode("utf-8") for t in texts]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
    ids, oo = hutoken_amd.encode_packed_device(dev(np.frombuffer(b"".join(raw), dtype=np.uint8).copy()), dev(offs))
    oa, ob = oo[:n + 1], oo[n:]
    assert ob.data_ptr() % 16 == 8 and int(ob[0].item()) > 0
    docs = hutoken_amd.batch_encode(texts)
    host_ids, host_oo = ids.cpu().numpy(), oo.cpu().numpy()
    assert [host_ids[host_oo[i]:host_oo[i + 1]].tolist() for i in range(2 * n)] == docs
    tpl = dict(bos_id=1, sep_ids=(4,), eos_id=2)
    d = (ids, oa, ids, ob)
    for strategy in R.STRATEGIES:
        for L in (31, 32):
            check(host_ids, host_oo[:n + 1], host_ids, host_oo[n:], L, strategy, d=d, **tpl)
            if strategy != "longest_first":
                check_windows(host_ids, host_oo[:n + 1], host_ids, host_oo[n:], L, 5, strategy, d=d, **tpl)
    a, oa2 = R.ragged(docs[:n])  # and against the reference on the two lists, each with offsets from 0
    b, ob2 = R.ragged(docs[n:])
    got = [g.cpu().numpy() for g in hutoken_amd.collate_pair_windows(*d, 32, 5, check=True, **tpl)]
    assert all(same(g, w) for g, w in zip(got, R.pair_windows(a, oa2, b, ob2, 32, 5, **tpl)))
    assert torch.equal(hutoken_amd.collate_pairs(*d, check=True, **tpl)[3],
                       dev((np.diff(oa2) + np.diff(ob2) + 3).astype(np.int32)))  # max_length=None: nothing is cut


def test_views_off_the_16_byte_boundary():
    import torch
    from hutoken_amd import _capi
    rng = np.random.default_rng(21)
    n = 300
    la, lb = random_lens(rng, n, 64), random_lens(rng, n, 64)
    both, oo = ragged_from(np.concatenate([la, lb]), rng, base=0)
    kw = TEMPLATES[2]
    for in_shift in (0, 1):
        d_ids = dev(np.concatenate([np.zeros(in_shift, dtype=np.int32), both]))[in_shift:]
        d_oo = dev(np.concatenate([np.zeros(in_shift, dtype=np.int64), oo]))[in_shift:]
        d = (d_ids, d_oo[:n + 1], d_ids, d_oo[n:])
        assert d_ids.data_ptr() % 16 == 4 * in_shift
        for dtype in (torch.int32, torch.int64):
            np_dtype = np.int64 if dtype == torch.int64 else np.int32
            for flags in (0, _capi.COLLATE_PAD_LEFT):
                side = "left" if flags else "right"
                for shift in (0, 1):
                    got = raw_pairs(d, 64, 0, _capi.PAIR_LONGEST_FIRST, kw, flags, dtype, shift, False)
                    assert got[0].data_ptr() % 16 == (0 if shift == 0 else dtype.itemsize)
                    want = R.pairs_vec(both, oo[:n + 1], both, oo[n:], 64, "longest_first", pad_id=PAD, padding_side=side,
                                       dtype=np_dtype, **kw)
                    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, want))
                    assert torch.equal(got[4], torch.stack([torch.arange(n), torch.zeros(n, dtype=torch.int64)], 1).to("cuda:0"))
                    got = raw_pairs(d, 64, 22, _capi.PAIR_ONLY_SECOND, kw, flags, dtype, shift, True)
                    want = R.pair_windows_vec(both, oo[:n + 1], both, oo[n:], 64, 22, "only_second", pad_id=PAD,
                                              padding_side=side, dtype=np_dtype, **kw)
                    assert all(same(g.cpu().numpy(), w) for g, w in zip(got[1:], want))
    # without the optional outputs
    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros((n, 64), dtype=torch.int32, device="cuda:0")
    _capi.collate_pairs_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 0, n, d_ids.numel(),
                               d_ids.numel(), n, 64, 0, _capi.PAIR_ONLY_FIRST, kw["bos_id"], kw["sep_ids"], kw["eos_id"], PAD, 0, 4,
                               out.data_ptr(), 0, 0, 0, 0, 0, st)
    assert same(out.cpu().numpy(), R.pairs_vec(both, oo[:n + 1], both, oo[n:], 64, "only_first", pad_id=PAD, **kw)[0])


def sanitised(ids, offs):
    """the documents as the kernels read offsets outside their condition: such a document is empty"""
    cap = len(ids)
    return [ids[o0:o1].tolist() if 0 <= o0 <= o1 <= cap else [] for o0, o1 in zip(offs[:-1].tolist(), offs[1:].tolist())]


def test_bad_offsets_are_range_checked_and_reported():
    """Every case is one the kernels range-check: nothing is read or written out of bounds, the documents concerned
    count as empty, their rows hold the other side, the template's tokens and padding."""
    import torch
    import hutoken_amd
    from hutoken_amd import _capi
    rng = np.random.default_rng(41)
    n = 100
    a, oa = ragged_from(rng.integers(0, 12, size=n), rng)
    b, ob = ragged_from(rng.integers(0, 60, size=n), rng)
    kw = dict(bos_id=1, sep_ids=(4,), eos_id=2)
    decreasing = ob.copy()
    decreasing[50] = decreasing[49] - 1 if decreasing[49] > 0 else decreasing[51] + 1
    assert (np.diff(decreasing) < 0).any()
    past = ob.copy()
    past[-3:] += 1000  # the last documents reach past numel
    negative = ob - 7  # a negative base
    huge = ob.copy()
    huge[10], huge[60] = 2**62, -2**62
    for name, bad in (("decreasing", decreasing), ("past", past), ("negative", negative), ("huge", huge)):
        docs_b = sanitised(b, bad)
        assert docs_b != sanitised(b, ob)
        sb, sob = R.ragged(docs_b)
        for side_b in (True, False):  # the bad offsets as B's, then as A's
            d = (dev(a), dev(oa), dev(b), dev(bad)) if side_b else (dev(b), dev(bad), dev(a), dev(oa))
            ref = (a, oa, sb, sob) if side_b else (sb, sob, a, oa)
            for L in (15, 16):
                with pytest.raises(ValueError, match="collate_pairs"):
                    hutoken_amd.collate_pairs(*d, L, check=True, **kw)
                with pytest.raises(ValueError, match="collate_pair_windows"):
                    hutoken_amd.collate_pair_windows(*d, L, 3, check=True, **kw)
                for strategy in R.STRATEGIES:
                    got = raw_pairs(d, L, 0, getattr(_capi, "PAIR_" + strategy.upper()), kw, 0, torch.int32, L % 2, False, _capi.E_ARG)
                    want = R.pairs(*ref, L, strategy, pad_id=PAD, **kw)
                    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, want)), (name, side_b, L, strategy)
                    if strategy == "longest_first":
                        continue
                    got = raw_pairs(d, L, 3, getattr(_capi, "PAIR_" + strategy.upper()), kw, _capi.COLLATE_PAD_LEFT, torch.int64,
                                    L % 2, True, _capi.E_ARG)
                    want = R.pair_windows(*ref, L, 3, strategy, pad_id=PAD, padding_side="left", dtype=np.int64, **kw)
                    assert same(got[0].cpu().numpy(), R.row_offsets(ref[1], ref[3], L, 3, strategy, **kw))
                    assert all(same(g.cpu().numpy(), w) for g, w in zip(got[1:], want)), (name, side_b, L, strategy)
    # a row_offsets that is not the scan of the counts: reported, nothing outside the rectangle written (the guards)
    d = (dev(a), dev(oa), dev(b), dev(ob))
    ro = R.row_table(oa, ob, 16, 3, "only_second", **kw)[0]
    n_rows = int(ro[-1])
    st = torch.cuda.current_stream().cuda_stream
    for wrong in (np.concatenate([ro[:40], ro[40:-1] - 1, ro[-1:]]), np.concatenate([[0], np.full(n - 1, 5), ro[-1:]]),
                  np.concatenate([[0], ro[1:-1][::-1], ro[-1:]])):
        buf, out = guarded(n_rows * 16, torch.int32, 4, FILL["out"])
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        _capi.collate_pairs_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                   dev(wrong.astype(np.int64)).data_ptr(), n, len(a), len(b), n_rows, 16, 3,
                                   _capi.PAIR_ONLY_SECOND, 1, (4,), 2, PAD, 0, 4, out.data_ptr(), 0, 0, 0, 0, err.data_ptr(), st)
        assert int(err.item()) == _capi.E_ARG and guards_untouched(buf, out, FILL["out"])


def test_64_bit_indices():
    """One pair whose windows write 2^31 + 2048 elements: 2^20 + 1 rows of 2048, a step of one id."""
    import torch
    import hutoken_amd
    L, kw = 2048, dict(bos_id=1, sep_ids=(4,), eos_id=2)
    C = L - 3 - 5
    a, oa = ragged_from([5], np.random.default_rng(4))
    b, ob = ragged_from([C + 2**20], np.random.default_rng(5), base=3)
    d_a, d_oa, d_b, d_ob = dev(a), dev(oa), dev(b), dev(ob)
    got = hutoken_amd.collate_pair_windows(d_a, d_oa, d_b, d_ob, L, C - 1, check=True, **kw)
    assert got[0].shape == (2**20 + 1, L) and got[0].numel() == 2**31 + 2048 and got[0].dtype == torch.int32
    table = window_table(oa, ob, L, C - 1, "only_second", kw)
    assert len(table[0]) == 2**20 + 1
    for r0 in range(0, 2**20 + 1, 2**16):  # the reference's row table, expanded 65 536 rows at a time
        r1 = min(r0 + 2**16, 2**20 + 1)
        want = torch_rows(d_a, oa, d_b, ob, [x[r0:r1] for x in table], L, "right", np.int32, **kw)
        want += (torch.stack([dev(table[0][r0:r1]), dev(table[2][r0:r1])], dim=1),)
        compare([g[r0:r1] for g in got], want, r0)
        del want
    del got
    torch.cuda.empty_cache()


def test_asynchronous_on_a_non_default_stream():
    import torch
    import hutoken_amd
    rng = np.random.default_rng(51)
    a, oa = ragged_from(rng.integers(0, 20, size=20000), rng)
    b, ob = ragged_from(random_lens(rng, 20000, 48), rng, base=2)
    kw = dict(bos_id=1, sep_ids=(4,), eos_id=2)
    n_rows = int(R.row_table(oa, ob, 48, 16, "only_second", **kw)[0][-1])
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        d = (dev(a), dev(oa), dev(b), dev(ob))
        got = hutoken_amd.collate_pair_windows(*d, 48, 16, n_rows=n_rows, **kw)
        with torch.cuda.stream(torch.cuda.Stream(device="cuda:0")):  # the scratch's event orders the two streams
            more = hutoken_amd.collate_pair_windows(*d, 48, 0, truncation="only_first")
        one = hutoken_amd.collate_pairs(*d, 48, **kw)
        torch.cuda.synchronize()
    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, R.pair_windows_vec(a, oa, b, ob, 48, 16, **kw)))
    assert all(same(g.cpu().numpy(), w) for g, w in zip(more, R.pair_windows_vec(a, oa, b, ob, 48, 0, "only_first")))
    assert all(same(g.cpu().numpy(), w) for g, w in zip(one, R.pairs_vec(a, oa, b, ob, 48, **kw)))


def test_list_forms(vg_files):
    import hutoken_amd
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    questions = ["Who wrote it?", "", "What is a stride?", "Where?", "How many tokens fit a row of thirty-two?"]
    contexts = ["It was written by nobody in particular.", "An empty question.", " ".join(["A stride is the overlap."] * 20), "",
                "Cafe\u0301 au lait, re\u0301sume\u0301 and nai\u0308ve are spelt with combining marks here. " * 6]
    tpl = dict(bos_id=50256, sep_ids=(50256, 50256), eos_id=50256)
    for normalize in (None, "NFC"):
        ta, tb = ((questions, contexts) if normalize is None else
                  ([unicodedata.normalize(normalize, t) for t in questions], [unicodedata.normalize(normalize, t) for t in contexts]))
        a, oa = R.ragged(hutoken_amd.batch_encode(ta))
        b, ob = R.ragged(hutoken_amd.batch_encode(tb))
        assert max(np.diff(ob)) > 100
        if normalize:
            assert not np.array_equal(b, R.ragged(hutoken_amd.batch_encode(contexts))[0])  # the form matters here
        for strategy in R.STRATEGIES:
            got = hutoken_amd.batch_encode_pairs(questions, contexts, 32, normalize=normalize, truncation=strategy, check=True, **tpl)
            assert all(same(g.cpu().numpy(), w) for g, w in zip(got, R.pairs(a, oa, b, ob, 32, strategy, **tpl)))
        got = hutoken_amd.batch_encode_pairs(questions, contexts, normalize=normalize, dtype="int64", **tpl)  # the longest pair
        L = int(max(np.diff(oa) + np.diff(ob))) + 4
        assert all(same(g.cpu().numpy(), w) for g, w in zip(got, R.pairs(a, oa, b, ob, L, dtype=np.int64, **tpl)))
        got = hutoken_amd.batch_encode_pair_windows(questions, contexts, 32, 8, normalize=normalize, check=True, **tpl)
        want = R.pair_windows(a, oa, b, ob, 32, 8, **tpl)
        assert want[0].shape[0] > 10 and all(same(g.cpu().numpy(), w) for g, w in zip(got, want))
        got = hutoken_amd.batch_encode_pair_windows(contexts, questions, 32, 8, normalize=normalize, truncation="only_first",
                                                    padding_side="left", **tpl)
        want = R.pair_windows(b, ob, a, oa, 32, 8, "only_first", padding_side="left", **tpl)
        assert all(same(g.cpu().numpy(), w) for g, w in zip(got, want))
