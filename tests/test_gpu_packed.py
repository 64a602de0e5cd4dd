"""Packed rows for training on the GPU (k_collate_packed_ch, k_collate_flush_ch, k_cu_write, k_cu_gaps, k_packed_labels in
csrc/hutk_collate.hip) against tests/packed_ref.py, element by element.  The shapes are the smallest at which the kernels
can go wrong: a workgroup of the packer owns 2048 stream positions, 8 per thread, and takes the 16-byte path when the row
length is a multiple of 4 and every output is aligned; a workgroup of the cu_seqlens count owns hutk_debug_cu_tile()
elements.  Needs a real MI355X."""
import functools
import random

import numpy as np
import pytest

import chat_ref
import collate_ref as CR
import packed_ref as R
from hutoken_amd import _capi

pytestmark = pytest.mark.gpu

IGN = -100
PAD = 9
TOKENS = {0: (None, None), 1: (None, 2), 2: (1, 2)}  # s -> (bos, eos)
CHANNELS = {"a": ("int32", -1), "b": ("int64", IGN), "c": ("int32", 7, 2), "d": ("int64", -2**40, 2)}
REF_CHANNELS = [(np.int32, 1, -1), (np.int64, 1, IGN), (np.int32, 2, 7), (np.int64, 2, -2**40)]
RAW_CHANNELS = [(4, 1, -1), (8, 1, IGN), (4, 2, 7), (8, 2, -2**40)]
NAMES = tuple(CHANNELS)
ROWS = ("input_ids", "position_ids", "segment_ids")
SMALL_L = (1, 3, 4, 7)
ALL_L = SMALL_L + (64, 2048, 2052, 4100)
SENT = 0x5A


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to("cuda:0")  # (a copy: the shared expectations are read-only)


def values_of(ids):
    """four per-token arrays that follow from the ids, so that any piece of a batch carries its own"""
    ids = np.asarray(ids, dtype=np.int32)
    wide = ids.astype(np.int64)
    return [ids * 3 + 1, -wide - 2**33, np.stack([ids, ids + 7], axis=1).astype(np.int32).reshape(len(ids), 2),
            np.stack([wide * 2**32, -wide], axis=1).reshape(len(ids), 2)]


def batch(docs):
    ids, offs = CR.ragged(docs)
    return ids, offs, values_of(ids)


@functools.lru_cache(None)
def documents():
    """random lengths with empties, a run of 3000 empty documents at one place, one document longer than three spans"""
    rng = random.Random(11)
    lens = [rng.choice((0, 0, 1, 2, 5, 17, 40, 130, 300)) for _ in range(40)]
    lens[20:20] = [0] * 3000
    lens.insert(10, 3 * 2048 + 5)
    return batch([[rng.randrange(10, 50000) for _ in range(n)] for n in lens])


@functools.lru_cache(None)
def device_documents():
    ids, _offs, values = documents()
    return dev(ids), [dev(v) for v in values]


@functools.lru_cache(None)
def expected(L, s):
    """the restatement's rows of documents(), complete and flushed concatenated; computed once and never changed"""
    ids, offs, values = documents()
    bos, eos = TOKENS[s]
    p = R.Packer(L, bos, eos, PAD, channels=REF_CHANNELS)
    rows = R.cat([p.add(ids, offs, values), p.flush()])
    for v in [rows[k] for k in ROWS] + rows["channels"]:
        v.setflags(write=False)
    return rows


def host(parts):
    """the dicts of several add / flush calls of the package -> one in packed_ref's form"""
    import torch
    out = {k: torch.cat([p[k] for p in parts]).cpu().numpy() for k in ROWS}
    out["channels"] = [torch.cat([p[n] for p in parts]).cpu().numpy() for n in NAMES if n in parts[0]]
    return out


def assert_rows(got, want):
    pairs = [(k, got[k], want[k]) for k in ROWS] + [("channel %d" % c, g, w) for c, (g, w) in enumerate(zip(got["channels"], want["channels"]))]
    assert len(got["channels"]) == len(want["channels"])
    for name, g, w in pairs:
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
        assert bad.size == 0, "%s differs at flat element %d of %d: got %d, want %d" % (
            name, bad[0], g.size, g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


def feed(p, a, b):
    """documents a .. b - 1 of documents() into packer p, as views into the one device copy"""
    _ids, offs, _values = documents()
    d_ids, d_values = device_documents()
    o0, o1 = int(offs[a]), int(offs[b])
    return p.add(d_ids[o0:o1], dev(offs[a:b + 1] - o0), n_ids=o1 - o0, check=True,
                 channels={n: v[o0:o1] for n, v in zip(NAMES, d_values)})


def gpu_rows(L, s, cuts):
    import hutoken_amd as H
    bos, eos = TOKENS[s]
    n = len(documents()[1]) - 1
    edges = [0] + list(cuts) + [n]
    with H.SequencePacker(L, bos_id=bos, eos_id=eos, pad_id=PAD, channels=CHANNELS) as p:
        parts = [feed(p, a, b) for a, b in zip(edges[:-1], edges[1:])]
        parts.append(p.flush())
        assert p.pending == 0
    return host(parts)


# ---- channels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
@pytest.mark.parametrize("L", ALL_L)
def test_three_ways_to_feed_the_same_documents(L, s):
    n = len(documents()[1]) - 1
    want = expected(L, s)
    assert_rows(gpu_rows(L, s, ()), want)
    assert_rows(gpu_rows(L, s, (n // 2,)), want)
    if L in SMALL_L:
        assert_rows(gpu_rows(L, s, range(1, n)), want)


def test_output_shapes_and_dtypes():
    import torch
    import hutoken_amd as H
    ids, offs, values = batch([[10, 11, 12], [], [20, 21, 22, 23, 24, 25], [30]])
    with H.SequencePacker(4, eos_id=99, channels={"labels": (torch.int64, IGN), "spans": ("int32", 0, 2)}) as p:
        rows = p.add(dev(ids), dev(offs), channels={"labels": dev(ids.astype(np.int64)), "spans": dev(values[2])})
        rest = p.flush()
        none = p.flush()
    assert list(rows) == list(rest) == list(none) == ["input_ids", "position_ids", "segment_ids", "labels", "spans"]
    assert rows["labels"].dtype == torch.int64 and rows["spans"].dtype == torch.int32
    assert rows["labels"].shape == (3, 4) and rows["spans"].shape == (3, 4, 2)
    assert rest["labels"].shape == (1, 4) and rest["spans"].shape == (1, 4, 2)
    assert none["labels"].shape == (0, 4) and none["spans"].shape == (0, 4, 2)
    # the worked example of the header
    assert rows["labels"].tolist() == [[10, 11, 12, IGN], [IGN, 20, 21, 22], [23, 24, 25, IGN]]
    assert rest["labels"].tolist() == [[30, IGN, IGN, IGN]] and rest["input_ids"].tolist() == [[30, 99, 0, 0]]
    assert rest["spans"][0].tolist() == [[30, 37], [0, 0], [0, 0], [0, 0]]


@pytest.mark.parametrize("L,s", [(64, 1), (7, 2), (2052, 0)])
def test_carry(L, s):
    """an add that completes no row, one that does, flush with tokens pending, flush with nothing pending, the packer used
    again after a flush -- call by call against the restatement"""
    import hutoken_amd as H
    bos, eos = TOKENS[s]
    rng = random.Random(L)
    doc = lambda n: [rng.randrange(10, 50000) for _ in range(n)]  # noqa: E731
    steps = [[[], doc(1)], [doc(L + 3), doc(2)], "flush", "flush", [doc(1)], [doc(2 * L), [], doc(L - 1)], [doc(1)], "flush"]
    ref = R.Packer(L, bos, eos, PAD, channels=REF_CHANNELS)
    with H.SequencePacker(L, bos_id=bos, eos_id=eos, pad_id=PAD, channels=CHANNELS) as p:
        for i, step in enumerate(steps):
            if step == "flush":
                got, want = p.flush(), ref.flush()
            else:
                ids, offs, values = batch(step)
                got = p.add(dev(ids), dev(offs), check=True, channels={n: dev(v) for n, v in zip(NAMES, values)})
                want = ref.add(ids, offs, values)
            assert_rows(host([got]), want)
            assert p.pending == ref.pending, i
    assert steps[0] != "flush" and want["input_ids"].shape[0] == 1


@pytest.mark.parametrize("L", [7, 64, 2048])
def test_an_int32_channel_is_what_a_plain_packer_makes_of_the_values(L):
    import torch
    import hutoken_amd as H
    ids, offs, values = documents()
    d_ids, d_values = device_documents()
    d_offs = dev(offs)
    with H.SequencePacker(L, pad_id=PAD, channels={"a": ("int32", -1)}) as p, H.SequencePacker(L, pad_id=-1) as plain:
        rows, want = p.add(d_ids, d_offs, channels={"a": d_values[0]}), plain.add(d_values[0], d_offs)
        assert rows["a"].shape[0] > 0 and torch.equal(rows["a"], want["input_ids"])
        for k in ("position_ids", "segment_ids"):
            assert torch.equal(rows[k], want[k])
        rest, want = p.flush(), plain.flush()
        assert rest["a"].shape[0] == 1 and torch.equal(rest["a"], want["input_ids"])


def off_view(n, dtype, fill=None):
    """n elements on the GPU as a view one element behind a 16-byte boundary, sentinels around and (fill=None) inside"""
    import torch
    base = torch.full((n + 8,), SENT, dtype=dtype, device="cuda:0")
    view = base[1:1 + n]
    if fill is not None:
        view.copy_(torch.from_numpy(np.array(fill, order="C").reshape(-1)))
    assert view.data_ptr() % 16 == base.element_size()
    return base, view


def assert_guards(base, n):
    assert int(base[0]) == SENT and (base[1 + n:] == SENT).all(), "written outside the view"


def test_views_one_element_off_the_16_byte_boundary():
    """outputs and values that are misaligned views take the element path and give the same rows"""
    import torch
    L, s = 64, 1
    ids, offs, values = documents()
    want = expected(L, s)
    n_docs, n_ids = len(offs) - 1, len(ids)
    p = _capi.Packer(L, eos_id=TOKENS[s][1], pad_id=PAD, out_width=4, device=0, channels=RAW_CHANNELS)
    assert p.channel_count == 4
    n = p.rows(n_docs, n_ids)
    assert n == want["input_ids"].shape[0] - 1  # (a row is left for the flush)
    t32, t64 = torch.int32, torch.int64
    d_ids, d_offs = off_view(n_ids, t32, ids)[1], off_view(n_docs + 1, t64, offs)[1]
    d_vals = [off_view(v.size, t, v)[1] for v, t in zip(values, (t32, t64, t32, t64))]
    recs = (1, 1, 2, 2)
    got = []
    for rows in (n, 1):
        outs = [off_view(rows * L, t32) for _ in ROWS] + [off_view(rows * L * r, t) for r, t in zip(recs, (t32, t64, t32, t64))]
        ptrs = [v.data_ptr() for _b, v in outs]
        if rows == n:
            err = torch.ones(1, dtype=t32, device="cuda:0")
            assert p.add_channels(d_ids.data_ptr(), d_offs.data_ptr(), n_docs, n_ids, [v.data_ptr() for v in d_vals], ptrs[0],
                                  ptrs[1], ptrs[2], ptrs[3:], n, err.data_ptr(), 0) == n
        else:
            assert p.flush_channels(ptrs[0], ptrs[1], ptrs[2], ptrs[3:], 0) == 1
        torch.cuda.synchronize()
        assert rows == 1 or int(err.item()) == 0
        for (base, view), r in zip(outs, (1, 1, 1) + recs):
            assert_guards(base, rows * L * r)
        part = {k: outs[i][1].view(rows, L) for i, k in enumerate(ROWS)}
        part.update({name: outs[3 + c][1].view((rows, L) + ((2,) if recs[c] == 2 else ())) for c, name in enumerate(NAMES)})
        got.append(part)
    p.close()
    assert_rows(host(got), want)


@pytest.mark.parametrize("case", ["first is not 0", "last is not n_ids", "decreasing"])
@pytest.mark.parametrize("L,s", [(16, 1), (2048, 0)])
def test_hostile_offsets_are_reported(case, L, s):
    """the reads of ids and values are range-checked by construction; what the test asserts is the error word"""
    import hutoken_amd as H
    n = 3 * L + 5
    ids, _offs, values = batch([list(range(10, 10 + n))])
    offs = {"first is not 0": [1, n // 2, n], "last is not n_ids": [0, n // 2, n - 1], "decreasing": [0, n // 2, n // 4, n]}[case]
    bos, eos = TOKENS[s]
    with H.SequencePacker(L, bos_id=bos, eos_id=eos, channels=CHANNELS) as p:
        with pytest.raises(ValueError, match="device-side error 4"):
            p.add(dev(ids), dev(np.array(offs, dtype=np.int64)), n_ids=n, check=True,
                  channels={k: dev(v) for k, v in zip(NAMES, values)})
        p.flush()  # usable again after a flush
        ids, offs, values = batch([[10, 11, 12]] * L)
        rows = p.add(dev(ids), dev(offs), check=True, channels={k: dev(v) for k, v in zip(NAMES, values)})
        assert rows["input_ids"].shape[0] == 3 + s


def test_refusals_that_need_a_device():
    import torch
    import hutoken_amd as H
    ids, offs, values = batch([[10, 11, 12], [20, 21]])
    d_ids, d_offs = dev(ids), dev(offs)
    p = _capi.Packer(8, device=0, channels=[(4, 1, 0)])
    d_val = dev(values[0])
    out = torch.empty(8, dtype=torch.int32, device="cuda:0")
    assert p.add_channels(d_ids.data_ptr(), d_offs.data_ptr(), 2, 5, [d_val.data_ptr()], 0, 0, 0, [0], 0) == 0 and p.pending == 5
    # the calls without channels would lose the channels' carry: refused, nothing consumed
    with pytest.raises(TypeError, match="has channels"):
        p.add(d_ids.data_ptr(), d_offs.data_ptr(), 2, 5, out.data_ptr(), 0, 0, 1)
    with pytest.raises(TypeError, match="has channels"):
        p.flush(out.data_ptr(), 0, 0)
    assert p.pending == 5
    with pytest.raises(TypeError, match="d_values and d_channel_rows must be given"):
        p.flush_channels(out.data_ptr(), 0, 0, [])
    with pytest.raises(TypeError, match="buffer is NULL"):
        p.flush_channels(out.data_ptr(), 0, 0, [0])
    assert p.pending == 5
    ch = torch.empty(8, dtype=torch.int32, device="cuda:0")
    assert p.flush_channels(out.data_ptr(), 0, 0, [ch.data_ptr()]) == 1
    assert out.tolist() == [10, 11, 12, 20, 21, 0, 0, 0] and ch.tolist() == values[0].tolist() + [0, 0, 0]
    p.close()
    # a packer without channels: the new calls are the old ones
    q = _capi.Packer(4, device=0)
    assert q.channel_count == 0
    assert q.add_channels(d_ids.data_ptr(), d_offs.data_ptr(), 2, 5, [], out.data_ptr(), 0, 0, [], 1) == 1
    assert q.flush_channels(out[4:].data_ptr(), 0, 0, []) == 1
    assert out.tolist() == [10, 11, 12, 20, 21, 0, 0, 0]
    q.close()
    with H.SequencePacker(8, channels={"a": ("int32", 0)}) as sp:
        with pytest.raises(ValueError, match="fewer than n_ids = 5"):
            sp.add(d_ids, d_offs, channels={"a": d_val[:4]})
        with pytest.raises(ValueError, match="must be on the device of ids"):
            sp.add(d_ids, d_offs, channels={"a": d_val.cpu()})
        assert sp.pending == 0


# ---- cu_seqlens ----------------------------------------------------------------------------------------------------------
def cu_check(seg, cap=None, view=False):
    """packed_cu_seqlens on seg against the restatement, max_seqlen included -> n_seq"""
    import torch
    import hutoken_amd as H
    seg = np.ascontiguousarray(seg, dtype=np.int32)
    d_seg = off_view(seg.size, torch.int32, seg)[1].view(seg.shape) if view else dev(seg)
    n_seq = R.cu_seqlens_vec(seg, 0)[1][0]
    want_cu, want_info = R.cu_seqlens_vec(seg, n_seq if cap is None else cap)
    cu, info = H.packed_cu_seqlens(d_seg, cap=cap)
    assert cu.dtype == torch.int32 and info.dtype == torch.int32 and info.shape == (2,)
    assert cu.shape == want_cu.shape, (cu.shape, want_cu.shape)
    bad = np.nonzero(cu.cpu().numpy() != want_cu)[0]
    assert bad.size == 0, "cu_seqlens differs at %d of %d: got %d, want %d" % (bad[0], want_cu.size, int(cu[bad[0]]), want_cu[bad[0]])
    assert tuple(info.tolist()) == want_info
    return n_seq


@pytest.mark.parametrize("L,s", [(3, 0), (64, 1), (2052, 2), (4100, 1)])
def test_cu_seqlens_of_the_packers_rows(L, s):
    seg = expected(L, s)["segment_ids"]
    n_seq = cu_check(seg)
    cu_check(seg, cap=n_seq)
    cu_check(seg, cap=n_seq + 5)


def test_cu_seqlens_of_synthetic_segments():
    assert cu_check(np.ones((37, 64))) == 37                                   # all equal: one sequence per row
    assert cu_check(np.tile(np.arange(513) % 2, (5, 1))) == 5 * 513            # alternating: every element starts one
    assert cu_check(np.arange(5000).reshape(5000, 1) % 3) == 5000              # L = 1: every row is one
    assert cu_check(np.full((5000, 1), 7), cap=5003) == 5000
    assert cu_check(np.zeros((0, 8)), cap=3) == 0 and cu_check(np.zeros((0, 8))) == 0
    assert cu_check(np.zeros((0, 8)), cap=0) == 0


def test_cu_seqlens_at_the_edges_of_a_workgroups_elements():
    T = _capi.cu_tile()
    n = 3 * T + 17  # not a multiple of the tile
    for deltas in ((-1,), (0,), (1,), (-1, 0, 1)):
        for rows, L in ((1, n), (n, 1)):
            step = np.zeros(n, dtype=np.int64)
            at = [k * T + d for k in (1, 2, 3) for d in deltas]
            step[at] = 1
            seg = np.cumsum(step).reshape(rows, L)
            n_seq = cu_check(seg, cap=n + 1)
            assert n_seq == (1 + len(at) if rows == 1 else n)
    # rows that end at, one before and one after the edge
    for L in (T - 1, T, T + 1):
        cu_check(np.ones((5, L)), cap=9)
        cu_check(np.tile(np.arange(L) // 700, (3, 1)))


def test_cu_seqlens_with_more_than_one_tile_per_workgroup():
    """above 4096 tiles a workgroup takes a whole number of tiles, and the chunks of its loop carry the count"""
    T = _capi.cu_tile()
    rng = np.random.default_rng(7)
    L = T + 1
    seg = np.repeat(rng.integers(0, 3, size=(4097, L // 16 + 1)), 16, axis=1)[:, :L]
    assert seg.size > 4096 * T
    cu_check(seg, cap=seg.size // 8)


def test_cu_seqlens_capacity():
    import torch
    import hutoken_amd as H
    seg = expected(64, 1)["segment_ids"]
    n_seq = R.cu_seqlens_vec(seg, 0)[1][0]
    total = seg.size
    cu_check(seg, cap=n_seq)                       # exactly enough
    cu, info = H.packed_cu_seqlens(dev(seg), cap=n_seq + 40, check=True)
    assert (cu[n_seq:] == total).all() and int(info[0]) == n_seq
    for cap in (n_seq - 1, 1, 0):
        cu_check(seg, cap=cap)                     # the first cap starts, then the total; the true count in info[0]
        with pytest.raises(ValueError, match=r"cap = %d is below the %d sequences" % (cap, n_seq)):
            H.packed_cu_seqlens(dev(seg), cap=cap, check=True)
    assert H.packed_cu_seqlens(dev(seg), cap=n_seq, check=True)[0].dtype == torch.int32


def test_cu_seqlens_of_a_misaligned_view():
    cu_check(expected(7, 2)["segment_ids"], view=True)
    cu_check(expected(64, 1)["segment_ids"], cap=5000, view=True)


# ---- labels ------------------------------------------------------------------------------------------------------------
def labels_check(values, seg, ignore=IGN):
    import hutoken_amd as H
    d_values, d_seg = dev(values), dev(np.ascontiguousarray(seg, dtype=np.int32))
    for shift in (False, True):
        got = H.packed_lm_labels(d_values, d_seg, shift=shift, ignore_index=ignore)
        want = R.labels_vec(values, seg, shift, ignore)
        assert got.dtype == d_values.dtype and got.shape == d_values.shape
        bad = np.nonzero(got.cpu().numpy().reshape(-1) != want.reshape(-1))[0]
        assert bad.size == 0, "labels (shift=%s) differ at %d: got %d, want %d" % (
            shift, bad[0], int(got.reshape(-1)[bad[0]]), want.reshape(-1)[bad[0]])


@pytest.mark.parametrize("L,s", [(3, 0), (7, 2), (64, 1), (2052, 2)])
def test_labels_of_the_packers_rows(L, s):
    rows = expected(L, s)
    labels_check(rows["input_ids"], rows["segment_ids"])
    labels_check(rows["input_ids"].astype(np.int64), rows["segment_ids"], ignore=-2**40)
    labels_check(rows["channels"][1], rows["segment_ids"], ignore=12345)
    labels_check(rows["channels"][0], rows["segment_ids"], ignore=-1)


def test_labels_of_small_and_padded_rows():
    rng = np.random.default_rng(5)
    labels_check(rng.integers(1, 99, size=(100, 1)).astype(np.int32), rng.integers(0, 2, size=(100, 1)))  # L = 1
    for L in (7, 64):
        seg = np.zeros((3, L), dtype=np.int32)
        seg[:, 0] = 1  # flushed rows that are all padding behind one token
        for dtype in (np.int32, np.int64):
            labels_check(rng.integers(1, 99, size=(3, L)).astype(dtype), seg)
    # any int32 is a segment id: a boundary is where two neighbours differ
    seg = rng.integers(-2, 3, size=(9, 260))
    labels_check(rng.integers(-2**62, 2**62, size=(9, 260)), seg, ignore=0)
    # the worked example of the header
    import hutoken_amd as H
    ids = np.array([[10, 11, 12, 99], [99, 20, 21, 22], [23, 24, 25, 99], [30, 99, 0, 0]], dtype=np.int32)
    seg = np.array([[1, 1, 1, 1], [1, 2, 2, 2], [1, 1, 1, 1], [1, 1, 0, 0]], dtype=np.int32)
    i = IGN
    assert H.packed_lm_labels(dev(ids), dev(seg), shift=True).tolist() == [[11, 12, 99, i], [i, 21, 22, i], [24, 25, 99, i], [99, i, i, i]]
    cu, info = H.packed_cu_seqlens(dev(seg), cap=8)
    assert cu.tolist() == [0, 4, 5, 8, 12, 14, 16, 16, 16] and info.tolist() == [6, 4]


@pytest.mark.parametrize("width", [4, 8])
def test_labels_on_misaligned_views(width):
    import torch
    rows = expected(64, 1)
    t = torch.int32 if width == 4 else torch.int64
    values, seg = rows["input_ids"].astype(np.int32 if width == 4 else np.int64), rows["segment_ids"]
    n_rows, L = seg.shape
    d_values, d_seg = off_view(seg.size, t, values)[1], off_view(seg.size, torch.int32, seg)[1]
    for shift in (False, True):
        base, out = off_view(seg.size, t)
        _capi.packed_labels_device(d_values.data_ptr(), width, d_seg.data_ptr(), n_rows, L, shift, 77, out.data_ptr(), 0)
        torch.cuda.synchronize()
        assert_guards(base, seg.size)
        assert np.array_equal(out.cpu().numpy().reshape(n_rows, L), R.labels_vec(values, seg, shift, 77))
    with pytest.raises(TypeError, match="must not overlap"):
        _capi.packed_labels_device(d_values.data_ptr(), width, d_seg.data_ptr(), n_rows, L, True, 77, d_values.data_ptr(), 0)


# ---- composition: conversations -> render -> one packer with channels -> labels and cu_seqlens ---------------------------
def test_chat_to_a_packed_training_batch():
    import torch
    import hutoken_amd as H
    rng = random.Random(3)
    parts = {"user": ([11, 12, 13], [14, 15]), "assistant": ([21], [22, 23], 1), "tool": ([], [])}
    ref_tpl = chat_ref.Template([[11, 12, 13], [21], []], [[14, 15], [22, 23], []], suffix_loss=[2, 1, 0], bos=1, eos=2)
    ids, offsets, roles, conv = [], [0], [], [0]
    for _ in range(60):
        for t in range(rng.randrange(0, 7)):
            ids += [rng.randrange(1000, 50000) for _ in range(rng.choice((0, 1, 3, 9, 40)))]
            offsets.append(len(ids))
            roles.append(rng.randrange(3))
        conv.append(len(roles))
    L = 32
    want = chat_ref.render(ref_tpl, ids, offsets, roles, conv, loss_roles=0b10, ignore_index=IGN)
    ref = R.Packer(L, pad_id=PAD, channels=[(np.int32, 1, IGN), (np.int32, 1, -1)])
    w_rows = R.cat([ref.add(want["out_ids"], want["out_offsets"], [want["labels"], want["turn_ids"]]), ref.flush()])
    w_labels = R.labels_vec(w_rows["channels"][0], w_rows["segment_ids"], True, IGN)
    n_seq = R.cu_seqlens_vec(w_rows["segment_ids"], 0)[1][0]
    w_cu, w_info = R.cu_seqlens_vec(w_rows["segment_ids"], n_seq)

    tpl = H.ChatTemplate(parts, bos_id=1, eos_id=2)
    t = lambda v, d: torch.tensor(v, dtype=d, device="cuda:0")  # noqa: E731
    out_ids, out_offsets, labels, turn_ids = H.render_chat_device(
        t(ids, torch.int32), t(offsets, torch.int64), t(conv, torch.int64), t(roles, torch.int32), tpl,
        loss_roles=("assistant",), return_turn_ids=True, check=True)
    with H.SequencePacker(L, pad_id=PAD, channels={"labels": ("int32", IGN), "turn_ids": ("int32", -1)}) as p:
        done = p.add(out_ids, out_offsets, check=True, channels={"labels": labels, "turn_ids": turn_ids})
        rest = p.flush()
    tpl.close()
    rows = {k: torch.cat([done[k], rest[k]]) for k in done}
    got = {k: rows[k].cpu().numpy() for k in ROWS}
    got["channels"] = [rows["labels"].cpu().numpy(), rows["turn_ids"].cpu().numpy()]
    assert_rows(got, w_rows)
    lab = H.packed_lm_labels(rows["labels"], rows["segment_ids"], shift=True)
    cu, info = H.packed_cu_seqlens(rows["segment_ids"])
    assert np.array_equal(lab.cpu().numpy(), w_labels) and (w_labels != IGN).any()
    assert np.array_equal(cu.cpu().numpy(), w_cu) and tuple(info.tolist()) == w_info
