"""Window collation on the GPU (csrc/hutk_collate.hip: k_windows_count, k_windows_write, k_collate_windows) against the
NumPy reference of tests/windows_ref.py, every comparison exact and over every element of all four outputs.

The loop form of the reference is used where it is fast enough, its vectorised form (pinned by the loop form in
tests/test_windows_cpu.py) up to NUMPY_MAX output elements.  Above that the reference's row table (every row's document,
start and length: windows_ref.row_table) is expanded to the rectangle on the device by torch_windows below, which every
smaller case pins against the NumPy forms first.  Needs a real MI355X."""
import numpy as np
import pytest

import windows_ref as R

pytestmark = pytest.mark.gpu

TOKENS = {0: {}, 1: {"eos_id": 50256}, 2: {"bos_id": -5, "eos_id": 50256}}
COMBOS = [(np.int32, "right"), (np.int64, "left"), (np.int32, "left"), (np.int64, "right")]
NUMPY_MAX = 3 << 19
LOOP_MAX = 3000  # ids


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def tdtype(dtype):
    import torch
    return torch.int64 if dtype == np.int64 else torch.int32


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def torch_windows(d_ids, offs, L, stride=0, bos_id=None, eos_id=None, pad_id=0, padding_side="right", dtype=np.int32):
    """windows_ref.windows_vec with the rectangle built on the device from windows_ref.row_table."""
    import torch
    s = (bos_id is not None) + (eos_id is not None)
    _ro, doc, start, n = R.row_table(offs, L, stride, bos_id, eos_id)
    doc, start, n, d_offs = dev(doc), dev(start), dev(n), dev(np.asarray(offs, dtype=np.int64))
    sl = n + s
    shift = L - sl if padding_side == "left" else torch.zeros_like(sl)
    q = torch.arange(L, device=doc.device)[None, :] - shift[:, None]
    valid = (q >= 0) & (q < sl[:, None])
    idx = d_offs[doc][:, None] + start[:, None] + q - int(bos_id is not None)
    src = torch.cat([d_ids, torch.zeros(1, dtype=torch.int32, device=doc.device)])
    out = torch.where(valid, src[idx.clamp_(0, src.numel() - 1)], torch.tensor(pad_id, dtype=torch.int32, device=doc.device))
    del idx
    if bos_id is not None:
        out = torch.where(q == 0, torch.tensor(bos_id, dtype=torch.int32, device=doc.device), out)
    if eos_id is not None:
        out = torch.where(q == sl[:, None] - 1, torch.tensor(eos_id, dtype=torch.int32, device=doc.device), out)
    return out.to(tdtype(dtype)), valid.to(torch.uint8), sl.to(torch.int32), torch.stack([doc, start], dim=1)


def check(ids, offs, L, stride, dtype=np.int32, side="right", pad_id=-9, label=None, **kw):
    """One collate_windows call against the reference: all four outputs, every element.  -> the device tensors."""
    import torch
    import hutoken_amd
    d_ids = dev(ids)
    got = hutoken_amd.collate_windows(d_ids, dev(offs), L, stride, dtype=tdtype(dtype), pad_id=pad_id, padding_side=side,
                                      check=True, **kw)
    label = (label, L, stride, kw, dtype, side)
    want = torch_windows(d_ids, offs, L, stride, pad_id=pad_id, padding_side=side, dtype=dtype, **kw)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), label
    if got[0].numel() <= NUMPY_MAX:
        host = [g.cpu().numpy() for g in got]
        assert all(same(g, w) for g, w in zip(host, R.windows_vec(ids, offs, L, stride, pad_id=pad_id, padding_side=side,
                                                                   dtype=dtype, **kw))), label
        if len(ids) <= LOOP_MAX and len(offs) <= LOOP_MAX:
            assert all(same(g, w) for g, w in zip(host, R.windows(ids, offs, L, stride, pad_id=pad_id, padding_side=side,
                                                                  dtype=dtype, **kw))), label
    return got


def strides(C):
    return sorted({0, 1, C // 2, C - 1} & set(range(C)))


def random_batch(seed, n_docs, L, C, step, n_long=2):
    """Document lengths from {0 .. 40} and a few of 1 k - 100 k ids, the latter cut to the length at which one document
    fills 2^18 output elements (with a step of 1 a document of 100 k ids is 100 k rows of L: a rectangle that tests
    nothing a shorter one does not and takes seconds to check); negative ids present."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, size=n_docs)
    if n_docs >= 2:
        for at in rng.integers(0, n_docs, size=min(n_long, n_docs)):
            lens[at] = min(int(rng.integers(1000, 100_001)), C + step * ((1 << 18) // L))
    offs = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(-3, 60000, size=int(offs[-1])).astype(np.int32)
    return ids, offs


@pytest.mark.parametrize("L", [1, 2, 7, 64, 100, 2048, 5000])  # 5000: column chunks; 7 and 100: element stores
@pytest.mark.parametrize("n_docs", [0, 1, 2, 63, 64, 65, 257, 5000])
def test_random_ragged_batches(n_docs, L):
    for s, kw in TOKENS.items():
        if L < s + 1:
            continue
        C = L - s
        for stride in strides(C):
            ids, offs = random_batch(1000 * n_docs + 10 * L + s, n_docs, L, C, C - stride)
            for dtype, side in COMBOS:
                check(ids, offs, L, stride, dtype, side, label=n_docs, **kw)


def edge_lengths(C, step):
    return [0, 1, C - 1, C, C + 1, C + step - 1, C + step, C + step + 1, C + 5 * step]


@pytest.mark.parametrize("C,step", [(1, 1), (2, 1), (2, 2), (5, 1), (5, 3), (5, 5), (7, 2), (64, 1), (64, 33), (64, 64)])
def test_lengths_on_every_edge_of_the_formula(C, step):
    rng = np.random.default_rng(C * 100 + step)
    lens = edge_lengths(C, step)
    for s, kw in TOKENS.items():
        L = C + s
        for dtype, side in COMBOS:
            for n in lens:  # single documents
                ids = rng.integers(-3, 60000, size=n).astype(np.int32)
                got = check(ids, np.array([0, n], dtype=np.int64), L, C - step, dtype, side, label=n, **kw)
                assert got[0].shape[0] == R.window_count(n, C, step)
            order = lens + lens[::-1]  # ... and as neighbours in one batch
            offs = np.concatenate([[0], np.cumsum(order)]).astype(np.int64)
            ids = rng.integers(-3, 60000, size=int(offs[-1])).astype(np.int32)
            check(ids, offs, L, C - step, dtype, side, label="neighbours", **kw)


def test_one_document_over_several_workgroups():
    ids = np.random.default_rng(3).integers(-3, 60000, size=100_000).astype(np.int32)
    offs = np.array([0, 100_000], dtype=np.int64)
    for dtype, side in COMBOS:
        got = check(ids, offs, 7, 5, dtype, side)
        assert got[0].shape == (49_998, 7)
    got = check(ids, offs, 8, 6, np.int32, "right")  # the 16-byte path: 49 997 rows
    assert got[0].shape == (49_997, 8)


@pytest.mark.parametrize("L", [7, 16])
def test_many_documents_in_one_workgroup(L):
    rng = np.random.default_rng(L)
    for lens in ([0] * 100_000 + [10_000], [10_000] + [0] * 100_000):
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ids = rng.integers(-3, 60000, size=10_000).astype(np.int32)
        for i, (dtype, side) in enumerate(COMBOS):
            check(ids, offs, L, 3, dtype, side, **TOKENS[i % 3])


def test_the_scan_across_blocks():
    """300 000 documents: more than one chunk of the scan over the workgroup sums (1024 workgroups of 256 documents)."""
    import torch
    from hutoken_amd import _capi
    n_docs, L, stride = 300_000, 16, 3
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 41, size=n_docs)
    offs = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(-3, 60000, size=int(offs[-1])).astype(np.int32)
    kw = TOKENS[1]
    want_ro = R.row_table(offs, L, stride, **kw)[0]
    d_offs = dev(offs)
    d_ro = torch.full((n_docs + 1,), -1, dtype=torch.int64, device="cuda:0")
    err = torch.ones(1, dtype=torch.int32, device="cuda:0")
    _capi.windows_rows_device(d_offs.data_ptr(), n_docs, len(ids), L, stride, _capi.NO_TOKEN, kw["eos_id"],
                              d_ro.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert int(err.item()) == 0
    assert np.array_equal(d_ro.cpu().numpy(), want_ro)
    got = [g.cpu().numpy() for g in check(ids, offs, L, stride, np.int32, "right", **kw)]
    edges = sorted({d + e for d in list(range(0, n_docs, 256)) + [n_docs - 1] for e in (-1, 0, 1)
                    if 0 <= d + e < n_docs})
    for d in edges:  # the rows of the documents on both sides of a boundary, by the loop form
        a, b = int(want_ro[d]), int(want_ro[d + 1])
        want = R.windows(ids[offs[d]:offs[d + 1]], np.array([0, lens[d]], dtype=np.int64), L, stride, pad_id=-9, **kw)
        want[3][:, 0] = d
        assert all(same(g[a:b], w) for g, w in zip(got, want)), d


def test_64_bit_indices():
    """One document, a step of one id: 2^20 + 1 rows of 2048, more than 2^31 elements."""
    import torch
    import hutoken_amd
    L, n = 2048, 2**20 + 2048
    d_ids = dev(np.random.default_rng(4).integers(-3, 60000, size=n).astype(np.int32))
    d_offs = dev(np.array([0, n], dtype=np.int64))
    out, mask, lengths, row_map = hutoken_amd.collate_windows(d_ids, d_offs, L, L - 1, check=True)
    assert out.shape == (2**20 + 1, L) and out.numel() == 2**31 + 2048 and out.dtype == torch.int32
    assert torch.equal(out, d_ids.unfold(0, L, 1))
    assert bool(mask.all()) and bool((lengths == L).all())
    assert torch.equal(row_map[:, 1], torch.arange(2**20 + 1, device="cuda:0")) and not bool(row_map[:, 0].any())
    del out, mask, lengths, row_map
    torch.cuda.empty_cache()


def raw_windows(d_ids, d_offs, n_ids, L, stride, bos, eos, pad, flags, dtype, shift):
    """The C ABI on views that begin `shift` elements into their buffers."""
    import torch
    from hutoken_amd import _capi
    n_docs = d_offs.numel() - 1
    st = torch.cuda.current_stream().cuda_stream
    d_ro = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda:0")
    err = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    _capi.windows_rows_device(d_offs.data_ptr(), n_docs, n_ids, L, stride, bos, eos, d_ro.data_ptr(), err.data_ptr(), st)
    n_rows = int(d_ro[-1].item())
    out = torch.zeros(n_rows * L + shift, dtype=dtype, device="cuda:0")[shift:]
    mask = torch.zeros(n_rows * L + shift, dtype=torch.uint8, device="cuda:0")[shift:]
    lengths = torch.zeros(n_rows + shift, dtype=torch.int32, device="cuda:0")[shift:]
    row_map = torch.zeros(2 * n_rows + shift, dtype=torch.int64, device="cuda:0")[shift:]
    _capi.collate_windows_device(d_ids.data_ptr(), d_offs.data_ptr(), d_ro.data_ptr(), n_docs, n_ids, n_rows, L, stride,
                                 bos, eos, pad, flags, dtype.itemsize, out.data_ptr(), mask.data_ptr(),
                                 lengths.data_ptr(), row_map.data_ptr(), err[1:].data_ptr(), st)
    assert not bool(err.any())
    return out.view(n_rows, L), mask.view(n_rows, L), lengths, row_map.view(n_rows, 2)


def test_unaligned_views_take_the_element_stores():
    import torch
    from hutoken_amd import _capi
    ids, offs = random_batch(21, 300, 64, 62, 40)
    d_ids, d_offs = dev(ids), dev(offs)
    for dtype in (torch.int32, torch.int64):
        for flags in (0, _capi.COLLATE_PAD_LEFT):
            a = raw_windows(d_ids, d_offs, len(ids), 64, 22, -5, 50256, -9, flags, dtype, 0)
            b = raw_windows(d_ids, d_offs, len(ids), 64, 22, -5, 50256, -9, flags, dtype, 1)
            assert a[0].data_ptr() % 16 == 0 and b[0].data_ptr() % 16 != 0
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            want = R.windows_vec(ids, offs, 64, 22, bos_id=-5, eos_id=50256, pad_id=-9,
                                 padding_side="left" if flags else "right", dtype=np.int64 if dtype == torch.int64 else np.int32)
            assert all(same(g.cpu().numpy(), w) for g, w in zip(b, want))
    # without the optional outputs
    st = torch.cuda.current_stream().cuda_stream
    d_ro = dev(R.row_table(offs, 64, 22, bos_id=-5, eos_id=50256)[0])
    n_rows = int(d_ro[-1].item())
    out = torch.zeros((n_rows, 64), dtype=torch.int32, device="cuda:0")
    _capi.collate_windows_device(d_ids.data_ptr(), d_offs.data_ptr(), d_ro.data_ptr(), len(offs) - 1, len(ids), n_rows, 64,
                                 22, -5, 50256, -9, 0, 4, out.data_ptr(), 0, 0, 0, 0, st)
    assert same(out.cpu().numpy(), R.windows_vec(ids, offs, 64, 22, bos_id=-5, eos_id=50256, pad_id=-9)[0])


def test_bad_offsets_are_reported_with_check():
    """Every case is one the kernels range-check: nothing is read or written out of bounds."""
    import hutoken_amd
    ids, offs = random_batch(31, 100, 16, 16, 13)
    d_ids, d_offs = dev(ids), dev(offs)
    good = hutoken_amd.collate_windows(d_ids, d_offs, 16, 3, check=True)
    n_rows = good[0].shape[0]
    assert n_rows == int(R.row_table(offs, 16, 3)[0][-1])
    bad = offs.copy()
    bad[0] = 1
    with pytest.raises(ValueError, match="device-side error 4"):  # offsets[0] != 0
        hutoken_amd.collate_windows(d_ids, dev(bad), 16, 3, n_ids=len(ids), check=True)
    with pytest.raises(ValueError, match="device-side error 4"):  # offsets[-1] != n_ids
        hutoken_amd.collate_windows(d_ids, d_offs, 16, 3, n_ids=len(ids) - 1, check=True)
    bad = offs.copy()
    bad[50] = bad[49] - 1 if bad[49] > 0 else bad[51] + 1  # a decreasing pair
    assert (np.diff(bad) < 0).any()
    with pytest.raises(ValueError, match="collate_windows"):
        hutoken_amd.collate_windows(d_ids, dev(bad), 16, 3, check=True)
    for off_by in (-1, 1):  # n_rows= that is not the number of rows
        with pytest.raises(ValueError, match="device-side error 4"):
            hutoken_amd.collate_windows(d_ids, d_offs, 16, 3, n_rows=n_rows + off_by, check=True)
    again = hutoken_amd.collate_windows(d_ids, d_offs, 16, 3, n_ids=len(ids), n_rows=n_rows, check=True)  # no read at all
    assert all(same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(again, good))


def test_asynchronous_on_a_non_default_stream():
    import torch
    import hutoken_amd
    ids, offs = random_batch(41, 20000, 48, 46, 30)
    n_rows = int(R.row_table(offs, 48, 16, bos_id=1, eos_id=2)[0][-1])
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        d_ids, d_offs = dev(ids), dev(offs)
        got = hutoken_amd.collate_windows(d_ids, d_offs, 48, 16, bos_id=1, eos_id=2, n_ids=len(ids), n_rows=n_rows)
        with torch.cuda.stream(torch.cuda.Stream(device="cuda:0")):  # the scratch's event orders the two streams
            more = hutoken_amd.collate_windows(d_ids, d_offs, 48, 0, n_ids=len(ids))
        torch.cuda.synchronize()
    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, R.windows_vec(ids, offs, 48, 16, bos_id=1, eos_id=2)))
    assert all(same(g.cpu().numpy(), w) for g, w in zip(more, R.windows_vec(ids, offs, 48, 0)))


def test_end_to_end_from_texts(vg_files):
    import hutoken_amd
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    rng = np.random.default_rng(6)
    words = ["window", " stride", " the", " overflow", " 12345", "\n", " tokens", " a", " mapping", "é"]
    texts = ["".join(words[i] for i in rng.integers(0, len(words), size=n))
             for n in [0, 1, 5, 23, 24, 25, 31, 32, 33, 100, 1000] + list(rng.integers(0, 120, size=200))]
    docs = hutoken_amd.batch_encode(texts)
    assert max(len(d) for d in docs) > 500 and min(len(d) for d in docs) == 0
    ids, offs = R.ragged(docs)
    got = [g.cpu().numpy() for g in hutoken_amd.batch_encode_windows(texts, 32, 8, eos_id=50256)]
    assert all(same(g, w) for g, w in zip(got, R.windows(ids, offs, 32, 8, eos_id=50256)))
    out, _mask, lengths, row_map = got
    for r in range(out.shape[0]):  # through row_map: every row's document ids are the stated slice of its document
        d, start = int(row_map[r, 0]), int(row_map[r, 1])
        n = int(lengths[r]) - 1
        assert out[r, :n].tolist() == docs[d][start:start + n] and out[r, n] == 50256
        assert start + n == len(docs[d]) or n == 31
