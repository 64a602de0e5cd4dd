"""Best-fit packing on the GPU against the restatement (tests/bestfit_ref.py): every output element by element, exact.
The C entry points run on buffers with sentinels around them, aligned (the 16-byte path where L % 4 == 0) and one
element off the 16-byte boundary (the element path); the Python functions on what torch allocates.
The document passes give every wavefront a run of per_wave documents, walked in chunks of 64 (include/hutoken_amd.h,
hutk_debug_bestfit_tile).  In the plan the sets of length_sets() stay at per_wave = 64, so their edges are those between
wavefronts and workgroups; test_wavefronts_that_walk_several_chunks and test_seq_len_65536 have per_wave = 128, where the
rank of an item and the whole rows in front of a document are carried from chunk to chunk.  The rows call's passes own
128 documents at least, so every set of more than 64 documents carries there.
Needs a real MI355X."""
import functools
import random

import numpy as np
import pytest

import bestfit_ref as R
import chat_ref
import packed_ref
from hutoken_amd import _capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 0x5A
PAD = 9
IGN = -100
TOKENS = {0: (None, None), 1: (None, 2), 2: (1, 2)}  # s -> (bos, eos)
ALL_L = (1, 2, 3, 4, 7, 8, 64, 2048, 2052)
ROWS = ("input_ids", "position_ids", "segment_ids", "lengths", "source")
E_ARG, E_CAPACITY = 4, 7


def tok(v):
    return _capi.NO_TOKEN if v is None else v


def ragged(lens, seed=1):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
    return rng.integers(10, 50000, size=int(offs[-1]), dtype=np.int32), offs


@functools.lru_cache(None)
def length_sets(L):
    """name -> document lengths: the sets the issue names, sized by L"""
    rng = random.Random(L)
    tile = _capi.bestfit_tile()
    mixed = [rng.choice((0, 0, 1, 2, 5, L // 3, L // 2, L - 1, L, L + 1)) for _ in range(40)]
    mixed[20:20] = [0] * 3000
    # (sequences of exactly L, 2L and 3L + 5 for every s: the lengths less 0, 1 and 2)
    mixed[10:10] = [3 * L + 5, L, 2 * L, max(L - 1, 0), max(L - 2, 0), 2 * L - 1, 2 * L - 2, 3 * L + 4, 3 * L + 3]
    sets = {
        "mixed": mixed,
        "all empty": [0] * 70,
        "no documents": [],
        "ties": [rng.choice((3, 3, 3, 5, max(L // 4, 1))) % (L + 1) for _ in range(300)],
        "one class": [max(L // 3, 1)] * 100,
        # every class above L / 2 for every s: sequence lengths L // 2 - 2 + s .. L + s
        "upper": [l for l in range(max(L // 2 - 2, 0), L + 1) for _ in range(2)],
        # more documents than two tiles of the ranking pass, equal lengths across every wavefront and tile edge
        "tiles": [rng.choice((1, 2, 2, 3, max(L // 5, 1), max(L // 2, 1))) for _ in range(2 * tile + 150)],
    }
    if L == 8:
        sets["split"] = [5, 5, 5, 3, 3, 3, 3, 2]  # a class that ends in the middle of a group, one in the middle of a bin
    return sets


@functools.lru_cache(None)
def batch(L, name):
    ids, offs = ragged(length_sets(L)[name], seed=len(name))
    ids.setflags(write=False)
    offs.setflags(write=False)
    return ids, offs


@functools.lru_cache(None)
def expected(L, s, name):
    """the restatement's rows (int32), computed once and never changed"""
    ids, offs = batch(L, name)
    bos, eos = TOKENS[s]
    want = R.pack(ids, offs, L, bos_id=bos, eos_id=eos, pad_id=PAD)
    for k in ROWS + ("doc_map",):
        want[k].setflags(write=False)
    return want


def guarded(n, dtype, off, fill=None):
    """n elements inside sentinels: 16-byte aligned, or (off) one element behind a 16-byte boundary"""
    import torch
    lead = 1 if off else 8
    base = torch.full((n + lead + 8,), SENT, dtype=dtype, device=DEV)
    view = base[lead:lead + n]
    if fill is not None:
        view.copy_(torch.from_numpy(np.array(fill, order="C").reshape(-1)))
    assert n == 0 or view.data_ptr() % 16 == (base.element_size() if off else 0)
    return base, view, lead


def whole(g, n=None):
    base, view, lead = g
    n = view.numel() if n is None else n
    return bool((base[:lead] == SENT).all()) and bool((base[lead + n:] == SENT).all())


def run(ids, offs, L, s, width=4, cap=None, off=False, edit=None, with_source=True):
    """the plan call and the rows call on guarded buffers -> (dict of numpy arrays, plan's error word, rows' error word);
    cap: rows_cap of both (None: the plan runs with the bound, the rows with info[0]); edit(doc_map tensor [n_docs, 4])
    runs between the two"""
    import torch
    bos, eos = TOKENS[s]
    n_docs, n_ids = len(offs) - 1, len(ids)
    t32, t64 = torch.int32, torch.int64
    d_ids, d_offs = guarded(n_ids, t32, off, ids)[1], guarded(n_docs + 1, t64, off, offs)[1]
    g_map, g_info = guarded(n_docs * 4, t64, off), guarded(2, t64, off)
    err = torch.ones(2, dtype=t32, device=DEV)
    plan_cap = _capi.bestfit_rows_bound(n_docs, n_ids, L, s) if cap is None else cap
    _capi.bestfit_plan_device(d_offs.data_ptr(), n_docs, n_ids, L, tok(bos), tok(eos), plan_cap, g_map[1].data_ptr(),
                              g_info[1].data_ptr(), err[0:].data_ptr(), 0)
    torch.cuda.synchronize()
    info = tuple(g_info[1].tolist())
    R_ = info[0] if cap is None else cap
    if edit is not None:
        edit(g_map[1].view(n_docs, 4))
    wt = t32 if width == 4 else t64
    outs = {"input_ids": guarded(R_ * L, wt, off), "position_ids": guarded(R_ * L, t32, off),
            "segment_ids": guarded(R_ * L, t32, off), "lengths": guarded(R_, t32, off)}
    if with_source:
        outs["source"] = guarded(R_ * L, t64, off)
    _capi.bestfit_rows_device(d_ids.data_ptr(), d_offs.data_ptr(), g_map[1].data_ptr(), n_docs, n_ids, L, tok(bos), tok(eos), PAD,
                              width, R_, outs["input_ids"][1].data_ptr(), outs["position_ids"][1].data_ptr(),
                              outs["segment_ids"][1].data_ptr(), outs["lengths"][1].data_ptr(),
                              outs["source"][1].data_ptr() if with_source else 0, err[1:].data_ptr(), 0)
    torch.cuda.synchronize()
    for k, g in list(outs.items()) + [("doc_map", g_map), ("info", g_info)]:
        assert whole(g), "%s: written outside the buffer" % k
    got = {k: g[1].cpu().numpy().reshape((R_, L) if k != "lengths" else (R_,)) for k, g in outs.items()}
    got["doc_map"] = g_map[1].cpu().numpy().reshape(n_docs, 4)
    got["info"] = info
    e = err.tolist()
    return got, e[0], e[1]


def assert_equal(got, want, what, keys=ROWS + ("doc_map",)):
    assert got["info"] == want["info"], what
    for k in keys:
        if k in got:
            assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
            bad = np.flatnonzero((got[k] != want[k]).reshape(-1))
            assert bad.size == 0, "%s: %s differs at flat %d: %d, want %d" % (what, k, bad[0], got[k].reshape(-1)[bad[0]],
                                                                             want[k].reshape(-1)[bad[0]])


@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("s", [0, 1, 2])
@pytest.mark.parametrize("L", ALL_L)
def test_rows_are_the_restatements(L, s, width):
    if L < s:
        with pytest.raises(TypeError, match="seq_len"):
            _capi.bestfit_plan_device(4096, 1, 1, L, 1, 2, 4, 4096, 4096)
        return
    for name in length_sets(L):
        ids, offs = batch(L, name)
        want = expected(L, s, name)
        got, e_plan, e_rows = run(ids, offs, L, s, width)
        assert (e_plan, e_rows) == (0, 0), name
        assert got["input_ids"].dtype == (np.int32 if width == 4 else np.int64)
        assert_equal(got, want, "L %d s %d %s" % (L, s, name))


def per_wave(n_docs, L, rows=False):
    """the documents a wavefront owns, by the header's rule (rows: the rows call's passes)"""
    waves = 4096 if rows else max(1, 2 ** 21 // L)
    return max(128 if rows else 64, -(-(-(-n_docs // waves)) // 64) * 64)


@pytest.mark.parametrize("L,s", [(2048, 1), (2052, 0)])
def test_wavefronts_that_walk_several_chunks(L, s):
    """70 000 documents: every wavefront of the plan's and of the rows call's document passes owns 128 documents, two
    chunks.  A handful of lengths, so that equal lengths lie on both sides of every chunk edge inside a run and an item's
    rank is carried over it; documents with whole rows in the first and in the second chunk of a run, so that the
    whole rows in front of a document are too."""
    n_docs = 70000
    assert per_wave(n_docs, L) == 128 and per_wave(n_docs, L, rows=True) == 128 and _capi.bestfit_tile() == 256
    rng = random.Random(L)
    lens = [rng.choice((1, 2, 2, 3, 3, 3, 7, 7, 0, L // 3 if rng.random() < 0.1 else 5)) for _ in range(n_docs)]
    for at, n in ((10, 2 * L + 5), (70, L), (128 + 3, L + 1), (128 + 64, 3 * L), (128 + 127, L - s), (69000, 2 * L), (69999, L + 9)):
        lens[at] = n
    for at in (63, 64, 127, 128, 129, 191, 192, 255, 256):  # one length across the chunk, wavefront and workgroup edges
        lens[at] = 11
    ids, offs = ragged(lens, seed=L)
    bos, eos = TOKENS[s]
    want = R.pack(ids, offs, L, bos_id=bos, eos_id=eos, pad_id=PAD)
    got, e_plan, e_rows = run(ids, offs, L, s)
    assert (e_plan, e_rows) == (0, 0)
    assert_equal(got, want, "70 000 documents, L %d" % L)


def test_seq_len_65536():
    """the largest seq_len: the walk's list heads lie in global memory, the rooms in use spread over every word of the
    bitmap's upper levels, and with 3 000 documents a wavefront of the plan owns 128 (at most 32 wavefronts)"""
    L, s, n_docs = 65536, 2, 3000
    assert per_wave(n_docs, L) == 128
    rng = random.Random(65536)
    big = (4096, 4097, 12000, 20000, 32766, 32767, 32768, 40000, 50000, 61000, 65533, 65534, 65535, 65536, 65536 + 9, 2 * 65536)
    lens = [rng.choice(big) if rng.random() < 0.04 else rng.randrange(1, 65536) if rng.random() < 0.01
            else rng.choice((0, 1, 2, 3, 3, 40, 40, 41, 600, 601, 1500)) for _ in range(n_docs)]
    ids, offs = ragged(lens, seed=3)
    want = R.pack(ids, offs, L, bos_id=1, eos_id=2, pad_id=PAD)
    first_rooms = {(L - (n + s) % L) >> 12 for n in lens if (n + s) % L > L // 2}  # a bin's room behind its first item
    assert len(first_rooms) >= 6 and want["info"][1] > 0, "rooms in several words of the bitmap's upper levels, and whole rows"
    got, e_plan, e_rows = run(ids, offs, L, s)
    assert (e_plan, e_rows) == (0, 0)
    assert_equal(got, want, "L 65536")
    with pytest.raises(TypeError, match="seq_len"):
        _capi.bestfit_plan_device(4096, 1, 1, L + 1, 1, 2, 4, 4096, 4096)


@pytest.mark.parametrize("L,s,name", [(8, 1, "mixed"), (8, 1, "split"), (64, 2, "tiles"), (7, 0, "mixed"), (2052, 1, "mixed")])
def test_views_one_element_off_the_16_byte_boundary(L, s, name):
    ids, offs = batch(L, name)
    for width in (4, 8):
        got, e_plan, e_rows = run(ids, offs, L, s, width, off=True)
        assert (e_plan, e_rows) == (0, 0)
        assert_equal(got, expected(L, s, name), "off by one element, L %d" % L)


@pytest.mark.parametrize("L,s", [(8, 1), (64, 0), (2048, 2)])
def test_capacity_equal_above_and_below(L, s):
    ids, offs = batch(L, "mixed")
    bos, eos = TOKENS[s]
    n_rows = expected(L, s, "mixed")["info"][0]
    for cap in (n_rows, n_rows + 3):
        want = R.pack(ids, offs, L, bos_id=bos, eos_id=eos, pad_id=PAD, rows_cap=cap)
        got, e_plan, e_rows = run(ids, offs, L, s, cap=cap)
        assert (e_plan, e_rows) == (0, 0)
        assert_equal(got, want, "cap %d of %d" % (cap, n_rows))
    for cap in (n_rows - 1, 1, 0):
        got, e_plan, e_rows = run(ids, offs, L, s, cap=cap)  # (run asserts that the sentinels are whole)
        assert e_plan == E_CAPACITY and got["info"] == expected(L, s, "mixed")["info"]
        assert cap == 0 or e_rows == E_ARG


def test_hostile_offsets_are_reported():
    L, s = 8, 1
    n = 3 * L + 5
    ids = np.arange(10, 10 + n, dtype=np.int32)
    for offs in ([0, n // 2, n // 4, n], [0, n // 2, n + 7, n], [1, n // 2, n], [0, n // 2, n - 1], [0, -4, n], [0, 2 * n, n]):
        for L_ in (L, 2048):
            got, e_plan, e_rows = run(ids, np.array(offs, dtype=np.int64), L_, s, cap=12, off=L_ == L)
            assert e_plan == E_ARG and e_rows == E_ARG, offs


def test_a_broken_doc_map_is_reported():
    L, s = 8, 1
    ids, offs = batch(L, "split")
    n_rows, W = expected(L, s, "split")["info"]

    def edits():
        yield lambda m: m[0, 2].fill_(n_rows + 5)     # a row behind the rows
        yield lambda m: m[0, 2].fill_(-7)
        yield lambda m: m[0, 2].fill_(2 ** 40)
        yield lambda m: m[1, 3].fill_(L)              # a column outside the row
        yield lambda m: m[1, 3].fill_(L - 1)          # an item that ends outside it
        yield lambda m: m[1, 3].fill_(-2)
        yield lambda m: m[2, 1].fill_(3)              # whole rows the document does not have
        yield lambda m: m[2, 0].fill_(0)
        yield lambda m: m[3, 2:].copy_(m[0, 2:])      # two items at one place
    for edit in edits():
        for off in (False, True):
            got, e_plan, e_rows = run(ids, offs, L, s, cap=n_rows, off=off, edit=edit)
            assert e_plan == 0 and e_rows == E_ARG
    long_ids, long_offs = batch(L, "mixed")
    got, e_plan, e_rows = run(long_ids, long_offs, L, s, edit=lambda m: m[10, 0].fill_(2 ** 33))  # the 3L + 5 document's whole rows
    assert e_plan == 0 and e_rows == E_ARG
    assert_equal(got, expected(L, s, "mixed"), "whole rows do not go through doc_map", keys=ROWS)


def test_the_same_call_twice_gives_identical_tensors():
    import torch
    import hutoken_amd as H
    for L, name in ((64, "tiles"), (2048, "mixed"), (8, "ties")):
        ids, offs = batch(L, name)
        d_ids, d_offs = torch.from_numpy(np.array(ids)).to(DEV), torch.from_numpy(np.array(offs)).to(DEV)
        a = H.pack_best_fit(d_ids, d_offs, L, eos_id=2, pad_id=PAD, return_source=True, return_doc_map=True, check=True)
        b = H.pack_best_fit(d_ids, d_offs, L, eos_id=2, pad_id=PAD, return_source=True, return_doc_map=True, check=True)
        assert sorted(a) == sorted(ROWS + ("doc_map",))
        for k in a:
            assert torch.equal(a[k], b[k]), k
        assert_equal({k: v.cpu().numpy() for k, v in a.items()} | {"info": expected(L, 1, name)["info"]}, expected(L, 1, name), name)


def test_python_surface():
    import torch
    import hutoken_amd as H
    L, s = 64, 2
    ids, offs = batch(L, "mixed")
    want = expected(L, s, "mixed")
    n_rows = want["info"][0]
    d_ids, d_offs = torch.from_numpy(np.array(ids)).to(DEV), torch.from_numpy(np.array(offs)).to(DEV)
    kw = dict(bos_id=1, eos_id=2, pad_id=PAD)
    got = H.pack_best_fit(d_ids, d_offs, L, **kw)
    assert sorted(got) == sorted(ROWS[:4]) and got["input_ids"].dtype == torch.int32 and got["input_ids"].shape == (n_rows, L)
    for k in got:
        assert torch.equal(got[k].cpu(), torch.from_numpy(np.array(want[k]))), k
    got = H.pack_best_fit(d_ids, d_offs, L, dtype=torch.int64, n_ids=len(ids), n_rows=n_rows + 2, return_source=True, check=True, **kw)
    wide = R.pack(ids, offs, L, bos_id=1, eos_id=2, pad_id=PAD, rows_cap=n_rows + 2, dtype=np.int64)
    assert got["input_ids"].dtype == torch.int64
    for k in got:
        assert torch.equal(got[k].cpu(), torch.from_numpy(wide[k])), k
    with pytest.raises(ValueError, match="device-side error 7"):
        H.pack_best_fit(d_ids, d_offs, L, n_rows=n_rows - 1, check=True, **kw)
    H.pack_best_fit(d_ids, d_offs, L, n_rows=n_rows - 1, **kw)  # (without check: no exception, no synchronisation)
    bad = torch.tensor([0, 5, 3, len(ids)], dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="device-side error 4"):
        H.pack_best_fit(d_ids, bad, L, n_ids=len(ids), n_rows=40, check=True, **kw)
    side = torch.cuda.Stream(DEV)  # a stream of the caller's
    with torch.cuda.stream(side):
        got = H.pack_best_fit(d_ids, d_offs, L, n_rows=n_rows, **kw)
    side.synchronize()
    assert torch.equal(got["segment_ids"].cpu(), torch.from_numpy(np.array(want["segment_ids"])))
    empty = H.pack_best_fit(d_ids[:0], d_offs[:1], L, **kw)
    assert empty["input_ids"].shape == (0, L) and empty["lengths"].shape == (0,)


def test_list_form(tmp_path):
    import torch
    import helpers
    import hutoken_amd as H
    ents, sp = helpers.random_byte_vocab(1, n_merges=50)
    vp, spath = helpers.write_vocab(tmp_path, "v", ents, sp)
    H.initialize(vp, spath, None, True)
    texts = ["hello world " * k for k in (1, 0, 7, 2, 30)]
    enc = H.batch_encode(texts)
    ids = np.array([x for e in enc for x in e], dtype=np.int32)
    offs = np.cumsum([0] + [len(e) for e in enc]).astype(np.int64)
    want = R.pack(ids, offs, 16, eos_id=2, pad_id=PAD)
    got = H.batch_encode_best_fit(texts, 16, eos_id=2, pad_id=PAD, return_source=True, return_doc_map=True)
    for k in ROWS + ("doc_map",):
        assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k


# ---- gather_source ---------------------------------------------------------------------------------------------------
RECORDS = [("int32", 1, -1), ("int64", 1, IGN), ("int32", 2, 7), ("int64", 2, -2 ** 40)]


def gather_ref(source, values, fill):
    out = np.full(source.shape + values.shape[1:], fill, dtype=values.dtype)
    ok = (source >= 0) & (source < len(values))
    out[ok] = values[source[ok]]
    return out


@pytest.mark.parametrize("dname,per,fill", RECORDS)
def test_gather_source_record_shapes(dname, per, fill):
    import torch
    import hutoken_amd as H
    rng = np.random.default_rng(per)
    n_values = 1000
    values = rng.integers(-2 ** 30, 2 ** 30, size=(n_values,) + ((2,) if per == 2 else ()), dtype=np.int64).astype(dname)
    if dname == "int64":
        values *= 2 ** 20
    for shape in ((37, 64), (5, 7), (1030,), (0, 8)):
        source = rng.integers(-1, n_values, size=shape, dtype=np.int64)
        want = gather_ref(source, values, fill)
        got = H.gather_source(torch.from_numpy(source).to(DEV), torch.from_numpy(values).to(DEV), fill, check=True)
        assert got.dtype == getattr(torch, dname) and torch.equal(got.cpu(), torch.from_numpy(want)), shape
        # guarded buffers, aligned and one element off: the C entry point
        n = source.size
        for off in (False, True):
            t = getattr(torch, dname)
            d_src, d_val = guarded(n, torch.int64, off, source)[1], guarded(values.size, t, off, values)[1]
            g_out = guarded(n * per, t, off)
            err = torch.ones(1, dtype=torch.int32, device=DEV)
            _capi.rows_gather_source_device(d_src.data_ptr(), n, d_val.data_ptr(), n_values, 4 if dname == "int32" else 8, per, fill,
                                            g_out[1].data_ptr(), err.data_ptr(), 0)
            torch.cuda.synchronize()
            assert whole(g_out) and int(err.item()) == 0
            assert np.array_equal(g_out[1].cpu().numpy().reshape(want.shape), want)
    # sources out of range: the fill and the error word; nothing is read outside the values
    source = np.array([0, n_values - 1, n_values, 2 ** 40, -1, -2 ** 40, 5, 2 ** 31], dtype=np.int64)
    got = H.gather_source(torch.from_numpy(source).to(DEV), torch.from_numpy(values).to(DEV), fill)
    assert torch.equal(got.cpu(), torch.from_numpy(gather_ref(source, values, fill)))
    with pytest.raises(ValueError, match="device-side error 4"):
        H.gather_source(torch.from_numpy(source).to(DEV), torch.from_numpy(values).to(DEV), fill, check=True)


def chat_case():
    rng = random.Random(3)
    ids, offsets, roles, conv = [], [0], [], [0]
    for _ in range(60):
        for t in range(rng.randrange(0, 7)):
            ids += [rng.randrange(1000, 50000) for _ in range(rng.choice((0, 1, 3, 9, 40)))]
            offsets.append(len(ids))
            roles.append(rng.randrange(3))
        conv.append(len(roles))
    return ids, offsets, roles, conv


def test_chat_to_best_fit_training_rows():
    """chat render -> pack_best_fit(return_source=True) -> gather_source(labels) -> packed_lm_labels and
    packed_cu_seqlens, against chat_ref, bestfit_ref and packed_ref; no conversation shorter than L is cut"""
    import torch
    import hutoken_amd as H
    ids, offsets, roles, conv = chat_case()
    L = 128
    parts = {"user": ([11, 12, 13], [14, 15]), "assistant": ([21], [22, 23], 1), "tool": ([], [])}
    ref_tpl = chat_ref.Template([[11, 12, 13], [21], []], [[14, 15], [22, 23], []], suffix_loss=[2, 1, 0], bos=1, eos=2)
    want = chat_ref.render(ref_tpl, ids, offsets, roles, conv, loss_roles=0b10, ignore_index=IGN)
    w_rows = R.pack(want["out_ids"], want["out_offsets"], L, pad_id=PAD)
    w_chan = gather_ref(w_rows["source"], want["labels"], IGN)
    w_turn_src = gather_ref(w_rows["source"], want["source"], -1)
    w_labels = packed_ref.labels_vec(w_chan, w_rows["segment_ids"], True, IGN)
    n_seq = packed_ref.cu_seqlens_vec(w_rows["segment_ids"], 0)[1][0]
    w_cu, w_info = packed_ref.cu_seqlens_vec(w_rows["segment_ids"], n_seq)

    tpl = H.ChatTemplate(parts, bos_id=1, eos_id=2)
    t = lambda v, d: torch.tensor(v, dtype=d, device=DEV)  # noqa: E731
    out_ids, out_offsets, labels, source = H.render_chat_device(
        t(ids, torch.int32), t(offsets, torch.int64), t(conv, torch.int64), t(roles, torch.int32), tpl,
        loss_roles=("assistant",), return_source=True, check=True)
    tpl.close()
    rows = H.pack_best_fit(out_ids, out_offsets, L, pad_id=PAD, return_source=True, return_doc_map=True, check=True)
    for k in ROWS + ("doc_map",):
        assert np.array_equal(rows[k].cpu().numpy(), w_rows[k]), k
    chan = H.gather_source(rows["source"], labels, IGN, check=True)
    assert np.array_equal(chan.cpu().numpy(), w_chan)
    # the render's own source array (content token -> index into the turns' ids), carried to the rows the same way
    assert np.array_equal(H.gather_source(rows["source"], source, -1, check=True).cpu().numpy(), w_turn_src)
    lab = H.packed_lm_labels(chan, rows["segment_ids"], shift=True)
    cu, info = H.packed_cu_seqlens(rows["segment_ids"])
    assert np.array_equal(lab.cpu().numpy(), w_labels) and (w_labels != IGN).any()
    assert np.array_equal(cu.cpu().numpy(), w_cu) and tuple(info.tolist()) == w_info
    # whole conversations: one shorter than L has no whole row and lies in one row, in one piece
    lens = np.diff(want["out_offsets"])
    dm = rows["doc_map"].cpu().numpy()
    short = (lens > 0) & (lens < L)
    assert short.sum() > 20 and (lens >= L).any()
    assert (dm[short, 1] == 0).all() and (dm[short, 2] >= 0).all() and (dm[short, 3] + lens[short] <= L).all()
    got_ids = rows["input_ids"].cpu().numpy()
    for i in np.flatnonzero(short):
        o0, o1 = want["out_offsets"][i], want["out_offsets"][i + 1]
        assert np.array_equal(got_ids[dm[i, 2], dm[i, 3]:dm[i, 3] + o1 - o0], want["out_ids"][o0:o1])


def test_more_than_2_to_the_31_output_elements():
    """int32 rows of L = 2048 whose flat index passes 2^31 among the whole rows of a long document, with every bin row
    behind it, and ids whose index passes 2^31 too.  Checked on the device against the restatement's plan."""
    import torch
    import hutoken_amd as H
    L, eos = 2048, 2
    rng = random.Random(7)
    long_rows = (400000, 300000, 348700)  # whole rows of the three long documents: 1 048 700 in all, 2^31 / L = 1 048 576
    lens = [rng.choice((0, 1, 5, 100, 700, 1500, 2047, 2048, 5000)) for _ in range(300)]
    for k, at in zip(long_rows, (3, 150, 290)):
        lens.insert(at, k * L + rng.choice((0, 17, 1200)))
    offs = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])
    n_docs, n_ids = len(lens), int(offs[-1])
    assert n_ids > 2 ** 31
    doc_map, seg, rooms, W = R.plan(offs, L, 1)
    n_rows = W + len(rooms)
    assert W * L > 2 ** 31 and len(rooms) > 50
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    ids = torch.randint(10, 50000, (n_ids,), dtype=torch.int32, device=DEV, generator=gen)
    d_offs = torch.from_numpy(offs).to(DEV)
    got = H.pack_best_fit(ids, d_offs, L, eos_id=eos, pad_id=PAD, n_ids=n_ids, n_rows=n_rows, return_source=True,
                          return_doc_map=True, check=True)
    assert got["input_ids"].numel() > 2 ** 31 and got["input_ids"].dtype == torch.int32
    assert torch.equal(got["doc_map"].cpu(), torch.from_numpy(doc_map))
    want_len = np.concatenate([np.full(W, L, dtype=np.int32), L - np.asarray(rooms, dtype=np.int32)])
    assert torch.equal(got["lengths"].cpu(), torch.from_numpy(want_len))
    flat = {k: got[k].view(-1) for k in ("input_ids", "position_ids", "segment_ids", "source")}
    real = 0
    for i in range(n_docs):
        o0, o1 = int(offs[i]), int(offs[i + 1])
        first, n_whole, row, col = (int(x) for x in doc_map[i])
        n_in = n_whole * L  # tokens of the sequence in whole rows: all of them ids unless the eos closes the last row
        if n_whole:
            a = first * L
            k = min(n_in, o1 - o0)
            assert torch.equal(flat["input_ids"][a:a + k], ids[o0:o0 + k]), i
            assert torch.equal(flat["source"][a:a + k], torch.arange(o0, o0 + k, device=DEV)), i
            if k < n_in:
                assert int(flat["input_ids"][a + k]) == eos and int(flat["source"][a + k]) == -1
            for r0 in range(first, first + n_whole, 65536):  # (in slices: a compare of a billion elements needs as many bytes)
                r1 = min(r0 + 65536, first + n_whole)
                assert bool((got["segment_ids"][r0:r1] == 1).all()), i
                assert bool((got["position_ids"][r0:r1] == torch.arange(L, device=DEV, dtype=torch.int32)).all()), i
            real += n_in
        if row >= 0:
            n = o1 - o0 + 1 - n_in
            a = row * L + col
            assert a > 2 ** 31
            assert torch.equal(flat["input_ids"][a:a + n - 1], ids[o0 + n_in:o1]) and int(flat["input_ids"][a + n - 1]) == eos, i
            assert torch.equal(flat["source"][a:a + n - 1], torch.arange(o0 + n_in, o1, device=DEV)) and int(flat["source"][a + n - 1]) == -1
            assert bool((flat["segment_ids"][a:a + n] == int(seg[i])).all()), i
            assert torch.equal(flat["position_ids"][a:a + n], torch.arange(n, device=DEV, dtype=torch.int32)), i
            real += n
    assert real == n_ids + n_docs  # every token of every sequence was looked at
    # the padding: everything else, as one count per array over the bin rows
    bins = slice(W, n_rows)
    n_pad = len(rooms) * L - int(want_len[W:].sum())
    assert int((got["segment_ids"][bins] == 0).sum()) == n_pad
    assert int(((got["input_ids"][bins] == PAD) & (got["segment_ids"][bins] == 0) & (got["position_ids"][bins] == 0)
                & (got["source"][bins] == -1)).sum()) == n_pad
