"""Collation on the GPU (csrc/hutk_collate.hip) against the NumPy reference of tests/collate_ref.py, every comparison exact
and over every element.  The loop form of the reference is used where it is fast enough, its vectorised form (pinned by the
loop form in tests/test_collate_cpu.py) everywhere.  Needs a real MI355X."""
import numpy as np
import pytest

import collate_ref as R

pytestmark = pytest.mark.gpu

TOKENS = {0: {}, 1: {"eos_id": 50256}, 2: {"bos_id": -5, "eos_id": 50256}}
SIDES = [("right", "right"), ("right", "left"), ("left", "right"), ("left", "left")]


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def tdtype(dtype):
    import torch
    return torch.int64 if dtype == np.int64 else torch.int32


def host(rows):
    return {k: v.cpu().numpy() for k, v in rows.items()}


def gpu_padded(ids, offs, L, dtype=np.int32, **kw):
    import hutoken_amd
    out = hutoken_amd.collate_padded(dev(ids), dev(offs), L, dtype=tdtype(dtype), check=True, **kw)
    return tuple(t.cpu().numpy() for t in out)


def piece(ids, offs, a, b):
    return ids[int(offs[a]):int(offs[b])], offs[a:b + 1] - offs[a]


def gpu_packed(ids, offs, L, cuts=(), dtype=np.int32, pad_id=0, **kw):
    """-> (complete rows of all add calls, flushed rows, pending after each call)"""
    import hutoken_amd
    n = len(offs) - 1
    cuts = [0] + list(cuts) + [n]
    parts, pend = [], []
    with hutoken_amd.SequencePacker(L, dtype=tdtype(dtype), pad_id=pad_id, **kw) as p:
        for a, b in zip(cuts[:-1], cuts[1:]):
            i, o = piece(ids, offs, a, b)
            parts.append(host(p.add(dev(i), dev(o), check=True)))
            pend.append(p.pending)
        tail = host(p.flush())
        assert p.pending == 0
        again = host(p.flush())
        assert again["input_ids"].shape == (0, L)
    return R.cat_rows(parts, L, dtype), tail, pend


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def random_batch(seed, n_docs, n_long=3):
    """Document lengths from {0 .. 40}, a few of 1 k - 100 k ids among them; negative ids present."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, size=n_docs)
    if n_docs >= 2:
        for at in rng.integers(0, n_docs, size=min(n_long, n_docs)):
            lens[at] = rng.integers(1000, 100_001)
    offs = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(-3, 60000, size=int(offs[-1])).astype(np.int32)
    return ids, offs


@pytest.mark.parametrize("L", [1, 2, 7, 64, 100, 2048])
@pytest.mark.parametrize("n_docs", [0, 1, 2, 63, 64, 65, 5000])
def test_random_ragged_batches(n_docs, L):
    ids, offs = random_batch(1000 * n_docs + L, n_docs)
    small = int(offs[-1]) < 30000
    for s, kw in TOKENS.items():
        for dtype in (np.int32, np.int64):
            whole, tail, _ = gpu_packed(ids, offs, L, dtype=dtype, pad_id=-9, **kw)
            vw, vt = R.packed_vec(ids, offs, L, pad_id=-9, dtype=dtype, **kw)
            assert R.rows_equal(whole, vw) and R.rows_equal(tail, vt), ("packed", s, dtype)
            if small:
                ref = R.Packer(L, pad_id=-9, dtype=dtype, **kw)
                assert R.rows_equal(whole, ref.add(ids, offs)) and R.rows_equal(tail, ref.flush())
            if L < max(1, s):
                continue
            for tr, side in SIDES:
                got = gpu_padded(ids, offs, L, dtype=dtype, pad_id=-9, truncation=tr, padding_side=side, **kw)
                want = R.padded_vec(ids, offs, L, pad_id=-9, truncation=tr, padding_side=side, dtype=dtype, **kw)
                assert all(same(g, w) for g, w in zip(got, want)), ("padded", s, dtype, tr, side)
                if small:
                    want = R.padded(ids, offs, L, pad_id=-9, truncation=tr, padding_side=side, dtype=dtype, **kw)
                    assert all(same(g, w) for g, w in zip(got, want))


def test_max_length_none_pads_to_the_longest_sequence():
    ids, offs = random_batch(77, 300, n_long=0)
    longest = int(np.diff(offs).max())
    for s, kw in TOKENS.items():
        got = gpu_padded(ids, offs, None, **kw)
        assert got[0].shape == (300, longest + s)
        assert all(same(g, w) for g, w in zip(got, R.padded_vec(ids, offs, longest + s, **kw)))
    got = gpu_padded(np.zeros(0, dtype=np.int32), np.zeros(4, dtype=np.int64), None)  # nothing but empty documents
    assert got[0].shape == (3, 1) and not got[1].any() and not got[2].any()


def check_both_layouts(ids, offs, Ls, token_sets, padded_L=64):
    for s in token_sets:
        kw = TOKENS[s]
        for L in Ls:
            for dtype in (np.int32, np.int64):
                whole, tail, _ = gpu_packed(ids, offs, L, dtype=dtype, **kw)
                vw, vt = R.packed_vec(ids, offs, L, dtype=dtype, **kw)
                assert R.rows_equal(whole, vw) and R.rows_equal(tail, vt), (s, L, dtype)
        for tr, side in SIDES:
            got = gpu_padded(ids, offs, padded_L, truncation=tr, padding_side=side, **kw)
            want = R.padded_vec(ids, offs, padded_L, truncation=tr, padding_side=side, **kw)
            assert all(same(g, w) for g, w in zip(got, want)), (s, tr, side)


def test_skew_one_giant_document_among_short_ones():
    rng = np.random.default_rng(3)
    lens = np.ones(100_001, dtype=np.int64)
    lens[61_234] = 3_000_000
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(-3, 60000, size=int(offs[-1])).astype(np.int32)
    check_both_layouts(ids, offs, [2048, 8192, 5001], [0, 1, 2])


def test_skew_a_run_of_empty_documents():
    rng = np.random.default_rng(4)
    lens = np.concatenate([rng.integers(0, 41, size=500), np.zeros(100_000, dtype=np.int64), rng.integers(0, 41, size=500),
                           np.zeros(100_000, dtype=np.int64)])
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(-3, 60000, size=int(offs[-1])).astype(np.int32)
    check_both_layouts(ids, offs, [7, 64, 2048, 8192, 30000], [0, 1])


def test_a_single_document_spanning_1000_rows():
    rng = np.random.default_rng(5)
    for L in (64, 2048, 4100):
        n = 1000 * L + 17
        ids = rng.integers(-3, 60000, size=n).astype(np.int32)
        offs = np.array([0, n], dtype=np.int64)
        for s in (0, 1, 2):
            whole, tail, _ = gpu_packed(ids, offs, L, **TOKENS[s])
            vw, vt = R.packed_vec(ids, offs, L, **TOKENS[s])
            assert len(whole["input_ids"]) == 1000 and R.rows_equal(whole, vw) and R.rows_equal(tail, vt)


@pytest.mark.parametrize("L", [3, 64, 2048, 4100, 8192])
def test_packer_over_several_adds_equals_one_add(L):
    ids, offs = random_batch(900 + L, 3000, n_long=4)
    n = len(offs) - 1
    rng = np.random.default_rng(L)
    for s, kw in TOKENS.items():
        one, tail1, _ = gpu_packed(ids, offs, L, **kw)
        vw, vt = R.packed_vec(ids, offs, L, **kw)
        assert R.rows_equal(one, vw) and R.rows_equal(tail1, vt)
        for n_adds in range(1, 8):
            cuts = sorted(rng.integers(0, n + 1, size=n_adds - 1).tolist())
            many, tail, pend = gpu_packed(ids, offs, L, cuts=cuts, **kw)
            assert R.rows_equal(many, one) and R.rows_equal(tail, tail1), (s, cuts)
            ends = cuts + [n]
            assert pend == [int(offs[e] + e * s) % L for e in ends], (s, cuts)


def test_small_documents_trickling_into_a_long_row():
    """Many adds that complete no row: the carry is copied forward and grows across spans of the kernel."""
    ids, offs = random_batch(11, 4000, n_long=0)
    cuts = list(range(37, 4000, 37))
    for L in (5000, 8192):
        for s in (0, 1):
            many, tail, _ = gpu_packed(ids, offs, L, cuts=cuts, **TOKENS[s])
            vw, vt = R.packed_vec(ids, offs, L, **TOKENS[s])
            assert R.rows_equal(many, vw) and R.rows_equal(tail, vt), (L, s)


def test_rows_cap_too_small_consumes_nothing():
    import torch
    from hutoken_amd import _capi
    ids, offs = random_batch(21, 500, n_long=1)
    L = 64
    a_i, a_o = piece(ids, offs, 0, 200)
    b_i, b_o = piece(ids, offs, 200, 500)
    p = _capi.Packer(L, eos_id=7)

    def add(i, o, cap=None):
        d_i, d_o = dev(i), dev(o)
        n = p.rows(len(o) - 1, len(i))
        cap = n if cap is None else cap
        out = {"input_ids": torch.empty((max(cap, 0), L), dtype=torch.int32, device="cuda:0"),
               "position_ids": torch.empty((max(cap, 0), L), dtype=torch.int32, device="cuda:0"),
               "segment_ids": torch.empty((max(cap, 0), L), dtype=torch.int32, device="cuda:0")}
        err = torch.ones(1, dtype=torch.int32, device="cuda:0")
        got = p.add(d_i.data_ptr(), d_o.data_ptr(), len(o) - 1, len(i), out["input_ids"].data_ptr(),
                    out["position_ids"].data_ptr(), out["segment_ids"].data_ptr(), cap, err.data_ptr(), 0)
        torch.cuda.synchronize()
        assert got == n and int(err.item()) == 0
        return host(out)

    first = add(a_i, a_o)
    pending = p.pending
    need = p.rows(300, len(b_i))
    assert need > 1
    with pytest.raises(RuntimeError, match="rows_cap"):
        add(b_i, b_o, cap=need - 1)
    assert p.pending == pending and p.rows(300, len(b_i)) == need
    second = add(b_i, b_o)
    want, _ = R.packed_vec(ids, offs, L, eos_id=7)
    assert R.rows_equal(R.cat_rows([first, second], L), want)
    p.close()


def test_offsets_that_disagree_with_n_ids_are_reported_through_d_err():
    import hutoken_amd
    ids, offs = random_batch(31, 100, n_long=0)
    d_ids, d_offs = dev(ids), dev(offs)
    with pytest.raises(ValueError, match="device-side error 4"):
        hutoken_amd.collate_padded(d_ids, d_offs, 16, n_ids=len(ids) - 1, check=True)
    bad = offs.copy()
    bad[0] = 1
    with pytest.raises(ValueError, match="device-side error 4"):
        hutoken_amd.collate_padded(d_ids, dev(bad), 16, n_ids=len(ids), check=True)
    with hutoken_amd.SequencePacker(16, eos_id=1) as p:
        with pytest.raises(ValueError, match="device-side error 4"):
            p.add(d_ids, d_offs, n_ids=len(ids) - 1, check=True)
        p.flush()  # usable again after a flush
        rows = host(p.add(d_ids, d_offs, check=True))
        assert R.rows_equal(rows, R.packed_vec(ids, offs, 16, eos_id=1)[0])


def test_asynchronous_on_a_non_default_stream():
    import torch
    import hutoken_amd
    ids, offs = random_batch(41, 20000, n_long=5)
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        d_ids, d_offs = dev(ids), dev(offs)
        padded = hutoken_amd.collate_padded(d_ids, d_offs, 48, bos_id=1, eos_id=2, n_ids=len(ids))
        with hutoken_amd.SequencePacker(2048, eos_id=2) as p:
            rows = p.add(d_ids, d_offs, n_ids=len(ids))
            with torch.cuda.stream(torch.cuda.Stream(device="cuda:0")):  # the packer's event orders the two streams
                tail = p.flush()
            torch.cuda.synchronize()
    want = R.padded_vec(ids, offs, 48, bos_id=1, eos_id=2)
    assert all(same(g.cpu().numpy(), w) for g, w in zip(padded, want))
    vw, vt = R.packed_vec(ids, offs, 2048, eos_id=2)
    assert R.rows_equal(host(rows), vw) and R.rows_equal(host(tail), vt)


def test_end_to_end_from_texts(vg_files, oracle_mod):
    import hutoken_amd
    from hutoken_amd import synth
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", 20000)
    texts = synth.docs_as_str(d, o)
    orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    ids, oo, _ = orc.encode_packed(d, o, 8)
    parts = []
    with hutoken_amd.SequencePacker(2048, eos_id=50256) as p:
        for a, b in ((0, 7000), (7000, 7001), (7001, 20000)):
            parts.append(host(p.add_texts(texts[a:b])))
        tail = host(p.flush())
    vw, vt = R.packed_vec(ids, oo, 2048, eos_id=50256)
    assert R.rows_equal(R.cat_rows(parts, 2048), vw) and R.rows_equal(tail, vt)
    got = hutoken_amd.batch_encode_padded(texts, 128, bos_id=50256, eos_id=50256, pad_id=0, dtype="int64")
    want = R.padded_vec(ids, oo, 128, bos_id=50256, eos_id=50256, pad_id=0, dtype=np.int64)
    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, want))
    got = hutoken_amd.batch_encode_padded(texts[:100])
    longest = int(np.diff(oo[:101]).max())
    want = R.padded_vec(ids, oo[:101], longest)
    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, want))


def test_full_size_every_element(vg_files):
    """C3, 1 M documents x VG, the ids as encode_packed_device leaves them on the device."""
    import torch
    import hutoken_amd
    from hutoken_amd import synth
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", 1_000_000)
    d_ids, d_oo = hutoken_amd.encode_packed_device(dev(d), dev(o))
    torch.cuda.synchronize()  # (on torch's default stream the encode runs on the context's own stream)
    oo = d_oo.cpu().numpy()
    n_ids = int(oo[-1])
    ids = d_ids[:n_ids].cpu().numpy()
    with hutoken_amd.SequencePacker(2048, eos_id=50256) as p:
        rows = p.add(d_ids, d_oo, n_ids=n_ids, check=True)
        tail = host(p.flush())
    rows = host(rows)
    vw, vt = R.packed_vec(ids, oo, 2048, eos_id=50256)
    assert R.rows_equal(rows, vw) and R.rows_equal(tail, vt)
    del rows, vw, vt
    got = hutoken_amd.collate_padded(d_ids, d_oo, 256, bos_id=50256, eos_id=50256, n_ids=n_ids, check=True)
    got = [g.cpu().numpy() for g in got]
    want = R.padded_vec(ids, oo, 256, bos_id=50256, eos_id=50256)
    assert all(same(g, w) for g, w in zip(got, want))
    torch.cuda.empty_cache()


def test_more_than_2_to_the_31_elements():
    """Padded, int32, n_docs x L just above 2^31: the first and last 1000 rows against the reference, the rest through
    sums taken on the device."""
    import torch
    import hutoken_amd
    L, n_docs = 2048, 2**20 + 1
    assert n_docs * L > 2**31
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 41, size=n_docs)
    lens[rng.integers(0, n_docs, size=50)] = 5000  # truncated rows
    offs = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    ids = rng.integers(-3, 60000, size=int(offs[-1])).astype(np.int32)
    out, mask, lengths = hutoken_amd.collate_padded(dev(ids), dev(offs), L, bos_id=1, eos_id=2, pad_id=-1,
                                                    truncation="left", check=True)
    assert out.numel() > 2**31 and out.shape == (n_docs, L)
    for a, b in ((0, 1000), (n_docs - 1000, n_docs)):
        want = R.padded_vec(ids, offs, L, bos_id=1, eos_id=2, pad_id=-1, truncation="left", rows=(a, b))
        assert same(out[a:b].cpu().numpy(), want[0]) and same(mask[a:b].cpu().numpy(), want[1])
        assert same(lengths[a:b].cpu().numpy(), want[2])
    kept = np.minimum(lens, L - 2)
    assert np.array_equal(lengths.cpu().numpy(), (kept + 2).astype(np.int32))
    csum = np.zeros(len(ids) + 1, dtype=np.int64)
    np.cumsum(ids, out=csum[1:], dtype=np.int64)
    want_sum = int((csum[offs[1:]] - csum[offs[1:] - kept]).sum()) + 3 * n_docs
    n_mask, total = 0, 0
    for a in range(0, n_docs, 65536):  # in pieces: no temporary the size of the output
        m = mask[a:a + 65536]
        n_mask += int(m.sum(dtype=torch.int64).item())
        total += int((out[a:a + 65536].to(torch.int64) * m).sum().item())
    assert n_mask == int(lengths.sum(dtype=torch.int64).item()) == int((kept + 2).sum())
    assert total == want_sum
    del out, mask, lengths
    torch.cuda.empty_cache()
