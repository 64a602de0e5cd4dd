"""Every device entry point on batches just past 2^31 and 2^32 bytes: byte positions, run and exception-list indices, id
positions, output offsets and chunk bases that are negative as int32 or wrap as uint32.

The batch is R copies of one block of documents (tests/wide_cases.py: an odd length of about 16 MiB, laid out so that
long words, a document boundary and a three-byte character straddle the place where each boundary falls).  The cases
with special tokens and byte fallback use a block of about 1 MiB laid out by the same rule, with a marker or an unknown
character across each boundary: specials_ref and fallback_ref walk the text byte by byte and id by id in Python, and the
positions a batch reaches do not depend on the block's length.  The split presets (the split and its listing, the encode
of a context with a preset, word ids) use that small block too, with a digit run, contractions and a whitespace run
across each boundary: presplit_ref is a Python loop as well.  The CPU references -- the oracle, decode_ref, spans_ref,
norm_ref, specials_ref, decode_special_ref, fallback_ref, presplit_ref, features_ref -- run on the block once; the
GPU's result for the batch is compared on the device, reshaped to [R, T], with the block's row, in slices, and never copied to the host.  A mismatch
names the copy, the byte position and the side of the boundary it is on.  Every case first asserts that the GPU on the
block alone equals the reference, so that a failure of the batch is one of position.

Memory: a case adds up what it allocates and what the context's workspace takes (include/hutoken_amd.h) and skips only
when torch.cuda.mem_get_info() shows less than 1.25 x that free; the skip names both numbers.  Every case prints one
line "WIDE | case | boundary | ran or skipped | bytes needed | bytes free | seconds" (pytest -s, or -rs for the skips).
Measured on an MI355X: the file 118 s, tests/test_gpu_bigdoc.py 18 s.  The byte-fallback encode is 46 s of that (16 s at
2^31, 30 s at 2^32, 9 s of the first for fallback_ref): it runs the token spans over the ids' CAPACITY, not their number.
The split presets' WIDE lines add up to 1.8 s (test_split_presets, six lines), 5.6 s (test_encode_under_a_preset, four)
and 4.8 s (test_word_ids, two).
Needs a real MI355X."""
import importlib

import numpy as np
import pytest

import decode_cases as DC
import decode_special_ref as DSR
import fallback_ref as F
import norm_ref as NR
import spans_ref as S
import specials_ref as SR
import wide_cases as W
from wide_cases import Row

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L = W.choose_length(16 * 2 ** 20 + 1, W.B31, W.B32, 2 ** 20, 2 ** 20)
L_SMALL = W.choose_length(2 ** 20 + 1, W.B31, W.B32)  # the block of the cases whose references are Python loops
BOUNDARIES = [pytest.param(W.B31, id="2GiB"), pytest.param(W.B32, id="4GiB")]
SLICE = 2 ** 28          # elements compared at a time: temporaries of a GiB at the most
SCRATCH = 3 * 2 ** 30    # what the comparisons themselves allocate
E_NUL_BYTE, E_WORD_TOO_LARGE, E_INVALID_UTF8 = 8, 9, 10
NOTE_OF_STATUS = {1: E_WORD_TOO_LARGE, 2: E_INVALID_UTF8}

_blocks = {}


def block(kind):
    if kind not in _blocks:
        _blocks[kind] = W.build(kind, L, W.B31, W.B32)
    return _blocks[kind]


def small_block(kind):
    if ("small", kind) not in _blocks:
        _blocks["small", kind] = W.build(kind, L_SMALL, W.B31, W.B32, rich=False)
    return _blocks["small", kind]


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def assert_rows(got, row, R, what, where, per_copy=L):
    W.assert_rows(got, row, R, what, where, per_copy, SLICE)


def assert_offsets(got, oo_block, R, what, where, per_copy=L):
    W.assert_offsets(got, oo_block, R, what, where, per_copy, SLICE)


class Batch:
    """R copies of a block on the device (data: the block's bytes with something written over them)"""

    def __init__(self, b, R, data=None):
        self.b, self.R, self.n_docs, self.n_bytes = b, R, R * len(b.docs), R * b.L
        self.bytes = dev(b.data if data is None else data).repeat(R)
        self.offs = dev(W.repeated_offsets(b.offs, b.L, R))
        assert self.bytes.numel() == self.n_bytes and self.bytes.data_ptr() % 16 == 0

    def doc_start(self, r, d):
        return r * self.b.L + int(self.b.offs[d])


def _context(name):
    from hutoken_amd import _capi, data
    files = data.vocab_files(name)
    vp, sp, kw = files
    return _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0), files


_oracle = {}


def oracle_rows(oracle_mod, name, kind, small=False):
    """(ids, out_offsets, status) of the CPU oracle for one block (small: the block of about 1 MiB), computed once"""
    if (name, kind, small) not in _oracle:
        from hutoken_amd import data
        vp, sp, kw = data.vocab_files(name)
        orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
        b = small_block(kind) if small else block(kind)
        ids, oo, st = orc.encode_packed(b.data, b.offs, 16)
        _oracle[name, kind, small] = (np.asarray(ids, dtype=np.int32), np.asarray(oo, dtype=np.int64), np.asarray(st, dtype=np.int32))
    return _oracle[name, kind, small]


def encode_need(ctx, n_bytes, n_docs):
    """text and offsets, ids at the capacity the call asks for, out_offsets and status, the context's workspace"""
    units = ctx.ids_capacity(1, 0) - 1
    return (n_bytes + 8 * (n_docs + 1) + 4 * ctx.ids_capacity(n_bytes, n_docs) + 12 * (n_docs + 1)
            + W.encode_workspace(n_bytes, n_docs, units) + SCRATCH)


def encode(ctx, bytes_, offs, n_docs, n_bytes, ids=None, how="plain"):
    """hutk_encode_batch_device (how: "special", "fallback": the entry points of those names) -> (ids at capacity,
    out_offsets, status, *d_err), synchronised"""
    import torch
    cap = (ctx.special_ids_capacity if how == "special" else ctx.ids_capacity)(n_bytes, n_docs)
    if ids is None:
        ids = torch.empty(cap, dtype=torch.int32, device=DEV)
    oo = torch.full((n_docs + 1,), -7, dtype=torch.int64, device=DEV)
    st = torch.full((max(n_docs, 1),), -7, dtype=torch.int32, device=DEV)
    err = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    text, out = (bytes_.data_ptr(), offs.data_ptr(), n_docs, n_bytes), (ids.data_ptr(), cap, oo.data_ptr(), st.data_ptr(),
                                                                       err.data_ptr(), stream())
    if how == "fallback":
        ctx.encode_fallback_device(*text, 0, *out)
    else:
        (ctx.encode_special_device if how == "special" else ctx.encode_device)(*text, *out)
    torch.cuda.synchronize()
    return ids, oo, st[:n_docs], int(err.item())


def assert_block_alone(b, got, want):
    """the GPU's (ids, out_offsets, status) for the block alone against the oracle's, naming the first document that differs"""
    (ids, oo, st), (ids_w, oo_w, st_w) = got, want
    n_got, n_want = np.diff(oo), np.diff(oo_w)
    bad = np.nonzero((n_got != n_want) | (st != st_w))[0]
    if bad.size == 0 and not np.array_equal(ids[:len(ids_w)], ids_w):
        k = int(np.nonzero(ids[:len(ids_w)] != ids_w)[0][0])
        bad = np.array([int(np.searchsorted(oo_w, k, side="right")) - 1])
    if bad.size:
        d = int(bad[0])
        raise AssertionError("the block alone differs from the oracle in %d documents (%s), first in document %d at byte %d, %d bytes "
                             "(%r): status %d and %d ids, the oracle has status %d and %d ids"
                             % (bad.size, bad[:8].tolist(), d, int(b.offs[d]), len(b.docs[d]), b.docs[d][:60], int(st[d]), int(n_got[d]),
                                int(st_w[d]), int(n_want[d])))
    assert np.array_equal(oo, oo_w)


def notes(st_block):
    """the error words a batch with these per-document statuses may leave: the first raised wins (atomicCAS from 0)"""
    return {NOTE_OF_STATUS[int(s)] for s in np.unique(st_block) if s} or {0}


# ---- 1. hutk_encode_batch_device ----------------------------------------------------------------------------------------
ENCODE_CONFIGS = [pytest.param("VG", "text", "0", id="VG-k_tiles"), pytest.param("VG", "cjk", "1", id="VG-cjk-k_ptiles"),
                  pytest.param("VL", "chars", None, id="VL-prefix")]


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("name,kind,ptiles", ENCODE_CONFIGS)
def test_encode(oracle_mod, monkeypatch, name, kind, ptiles, boundary):
    """ids, out_offsets, per-document status and *d_err of a batch past the boundary; then a NUL byte 12 345 bytes past the
    boundary is reported, and with the byte restored the next call on the same context is exact again."""
    if ptiles is not None:
        monkeypatch.setenv("HUTK_PTILES", ptiles)
    b = block(kind)
    ids_b, oo_b, st_b = oracle_rows(oracle_mod, name, kind)
    R = W.copies_cross(b.L, boundary)
    ctx, _files = _context(name)  # (before the memory rule: hutk_ids_capacity is the context's; it holds the tables only)
    try:
        with Row("encode %s %s%s" % (name, kind, " k_ptiles" if ptiles == "1" else ""), boundary, encode_need(ctx, R * b.L, R * len(b.docs))):
            assert ctx.tile_kernel(R * b.L) == (1 if ptiles == "1" else 0), "the batch would not be given the kernel this case is about"
            # the block alone
            ids, oo, st, err = encode(ctx, dev(b.data), dev(b.offs), len(b.docs), b.L)
            assert err in notes(st_b)
            assert_block_alone(b, (ids.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()), (ids_b, oo_b, st_b))
            del ids, oo, st
            # R copies
            batch = Batch(b, R)
            assert batch.n_bytes >= boundary + 2 ** 26
            T = len(ids_b)
            row_ids, row_st = dev(ids_b), dev(st_b)

            def id_pos(r, j):
                return batch.doc_start(r, int(np.searchsorted(oo_b, j, side="right")) - 1)

            def check(ids, oo, st, err, what):
                assert err in notes(st_b), "%s: *d_err = %d" % (what, err)
                assert_offsets(oo, oo_b, R, what + ", out_offsets", lambda r, d: batch.doc_start(r, d))
                assert_rows(st, row_st, R, what + ", status", lambda r, d: batch.doc_start(r, d))
                assert_rows(ids[:R * T], row_ids, R, what + ", ids", id_pos)

            ids, oo, st, err = encode(ctx, batch.bytes, batch.offs, batch.n_docs, batch.n_bytes)
            check(ids, oo, st, err, "%s %s" % (name, kind))
            # a NUL byte at a high position
            at = boundary + 12345
            while b.data[at % b.L] >= 0x80:  # (an ASCII byte: no character is torn, the NUL byte is the only error)
                at += 1
            keep = int(batch.bytes[at])
            batch.bytes[at] = 0
            _ids, _oo, _st, err = encode(ctx, batch.bytes, batch.offs, batch.n_docs, batch.n_bytes, ids)
            assert err == E_NUL_BYTE, "a NUL byte at position %d (%s): *d_err = %d" % (at, W.side(at), err)
            batch.bytes[at] = keep
            ids, oo, st, err = encode(ctx, batch.bytes, batch.offs, batch.n_docs, batch.n_bytes, ids)
            check(ids, oo, st, err, "%s %s, the call behind the refused one" % (name, kind))
            del ids, oo, st, _ids, _oo, _st, batch, row_ids, row_st
    finally:
        ctx.close()


# ---- 3. hutk_decode_batch_device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_decode(oracle_mod, vg_files, boundary):
    """The ids of case 1 (VG) back to text: the OUTPUT crosses the boundary, sizes call and write call."""
    import torch
    b = block("text")
    ids_b, oo_b, _st = oracle_rows(oracle_mod, "VG", "text")
    ref = DC.shipped_vocab_ref(vg_files)
    text_b, to_b = ref.decode_packed(ids_b, oo_b)
    assert not ref.status(ids_b, oo_b).any()
    T, TB, n = len(ids_b), len(text_b), len(b.docs)
    assert TB < b.L  # (the document with the over-long word is cut)
    R = W.copies_cross(TB, boundary)
    need = 4 * R * T + 8 * (R * n + 1) + R * TB + 12 * (R * n + 1) + R * T // 4 + SCRATCH
    ctx, _files = _context("VG")
    try:
        with Row("decode VG", boundary, need):
            def call(d_ids, d_io, nd, ni, out, cap):
                oo = torch.full((nd + 1,), -7, dtype=torch.int64, device=DEV)
                st = torch.full((nd,), -7, dtype=torch.int32, device=DEV)
                err = torch.full((1,), -7, dtype=torch.int32, device=DEV)
                torch.cuda.synchronize()
                ctx.decode_device(d_ids.data_ptr(), d_io.data_ptr(), nd, ni, out.data_ptr() if out is not None else 0, cap,
                                  oo.data_ptr(), st.data_ptr(), err.data_ptr(), stream())
                torch.cuda.synchronize()
                return oo, st, int(err.item())
            # the block alone
            out = torch.zeros(TB, dtype=torch.uint8, device=DEV)
            oo, st, err = call(dev(ids_b), dev(oo_b), n, T, out, TB)
            assert err == 0 and not st.any().item() and np.array_equal(oo.cpu().numpy(), to_b)
            assert np.array_equal(out.cpu().numpy(), text_b), "the block alone differs from decode_ref"
            # R copies
            d_ids = dev(ids_b).repeat(R)
            d_io = dev(W.repeated_offsets(oo_b, T, R))
            doc_at = lambda r, d: r * TB + int(to_b[d])  # noqa: E731  (positions in the OUTPUT text)
            oo, st, err = call(d_ids, d_io, R * n, R * T, None, 0)
            assert err == 0 and not st.any().item()
            assert_offsets(oo, to_b, R, "decode, the sizes call's out_offsets", doc_at, TB)
            total = int(oo[-1])
            assert total == R * TB >= boundary + 2 ** 26
            out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
            oo, st, err = call(d_ids, d_io, R * n, R * T, out, total)
            assert err == 0 and not st.any().item()
            assert_offsets(oo, to_b, R, "decode, out_offsets", doc_at, TB)
            assert_rows(out[:total], dev(text_b), R, "decode, text", lambda r, j: r * TB + j, TB)
            assert bool((out[total:] == 0xA5).all()), "written behind the output"
            del out, oo, st, d_ids, d_io
    finally:
        ctx.close()


# ---- 4. hutk_token_spans_device -----------------------------------------------------------------------------------------
_spans = {}


def span_rows(oracle_mod, vg_files, unit):
    """spans_ref on the small block: it walks every token in Python, half a minute for the two units on 16 MiB"""
    if unit not in _spans:
        b = small_block("text")
        ids_b, oo_b, _st = oracle_rows(oracle_mod, "VG", "text", small=True)
        tt = W.RefTokenText(DC.shipped_vocab_ref(vg_files))
        _spans[unit] = S.batch(tt, b.data, b.offs, ids_b, oo_b, True, unit, np.int64)
    return _spans[unit]


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_token_spans(oracle_mod, vg_files, boundary):
    """int64 spans in bytes and in characters (from 2^32 bytes on the character form takes its wide selection table),
    and int32 spans: refused for a DOCUMENT of 2^31 bytes, not for a batch of them."""
    import torch
    b = small_block("text")
    ids_b, oo_b, _st = oracle_rows(oracle_mod, "VG", "text", small=True)
    want = {u: span_rows(oracle_mod, vg_files, u) for u in ("byte", "char")}
    T, n = len(ids_b), len(b.docs)
    R = W.copies_cross(b.L, boundary)
    # (the spans' workspace, from csrc/hutk_spans.hip: two bitmaps of a bit per byte and a selection table of up to four
    # bytes per input byte)
    need = R * b.L + 16 * (R * n + 1) + 4 * R * T + 16 * R * T + 4 * R * n + 5 * R * b.L + SCRATCH
    ctx, _files = _context("VG")  # (holds the vocabulary's tables; the workspace grows with the first call)
    try:
        with Row("token spans VG", boundary, need):
            def call(d_bytes, d_offs, nd, nb, d_ids, d_io, ni, unit, width):
                out = torch.full((2 * ni,), -7, dtype=torch.int32 if width == 4 else torch.int64, device=DEV)
                st = torch.full((nd,), -7, dtype=torch.int32, device=DEV)
                err = torch.full((1,), -7, dtype=torch.int32, device=DEV)
                torch.cuda.synchronize()
                ctx.token_spans_device(d_bytes.data_ptr(), d_offs.data_ptr(), nd, nb, d_ids.data_ptr(), d_io.data_ptr(), ni,
                                       0 if unit == "byte" else 1, width, out.data_ptr(), st.data_ptr(), err.data_ptr(), stream())
                torch.cuda.synchronize()
                return out, st, int(err.item())
            for unit in ("byte", "char"):  # the block alone
                assert not want[unit][1].any()
                out, st, err = call(dev(b.data), dev(b.offs), n, b.L, dev(ids_b), dev(oo_b), T, unit, 8)
                assert err == 0 and not st.any().item()
                assert np.array_equal(out.cpu().numpy().reshape(T, 2), want[unit][0]), "the block alone differs from spans_ref (%s)" % unit
            batch = Batch(b, R)
            d_ids = dev(ids_b).repeat(R)
            d_io = dev(W.repeated_offsets(oo_b, T, R))

            def span_pos(r, j):
                return batch.doc_start(r, int(np.searchsorted(oo_b, j // 2, side="right")) - 1)
            for unit, width in (("byte", 8), ("char", 8), ("byte", 4), ("char", 4)):
                out, st, err = call(batch.bytes, batch.offs, batch.n_docs, batch.n_bytes, d_ids, d_io, R * T, unit, width)
                what = "spans in %ss, int%d" % (unit, 8 * width)
                assert err == 0, "%s: *d_err = %d for a batch of %d bytes whose longest document has %d" % (what, err, batch.n_bytes, int(np.diff(b.offs).max()))
                assert not st.any().item(), what
                row = dev(want[unit][0].astype(np.int32 if width == 4 else np.int64))
                assert_rows(out, row, R, what, span_pos, b.L)
                del out, st, row
            del batch, d_ids, d_io
    finally:
        ctx.close()


# ---- 5. hutk_normalize_batch_device -------------------------------------------------------------------------------------
_norm = {}


def norm_rows(form):
    if form not in _norm:
        _norm[form] = NR.reference(form, block("norm").docs)
    return _norm[form]


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("form", ["NFC", "NFKD"])
def test_normalize(form, boundary):
    """The sizes call and the write call: input AND output cross the boundary (chunk bases, out_offsets, the copy of
    clean chunks and the table path of the long runs of marks laid across both boundaries)."""
    import torch
    from hutoken_amd import _capi
    b = block("norm")
    out_b, oo_b, ch_b = norm_rows(form)
    assert ch_b.any() and not ch_b.all()
    n, TB = len(b.docs), len(out_b)
    R = W.copies_cross(min(b.L, TB), boundary)
    need = R * b.L + R * TB + 16 * (R * n + 1) + R * n + R * b.L // 64 + SCRATCH
    nz = _capi.Normalizer(importlib.import_module("hutoken_amd.normalize").table_blob(), 0)
    fi = NR.FORMS.index(form)
    try:
        with Row("normalize %s" % form, boundary, need):
            def run(d_bytes, d_offs, nd, nb):
                oo = torch.full((nd + 1,), -7, dtype=torch.int64, device=DEV)
                ch = torch.full((nd,), 7, dtype=torch.uint8, device=DEV)
                small = torch.full((4,), -7, dtype=torch.int64, device=DEV)  # the two totals; the error words of the two calls
                text = (fi, d_bytes.data_ptr(), d_offs.data_ptr(), nd, nb)
                torch.cuda.synchronize()
                nz.batch_device(*text, 0, 0, oo.data_ptr(), ch.data_ptr(), small.data_ptr(), small.data_ptr() + 16, stream())
                torch.cuda.synchronize()
                total, changed = int(small[0]), int(small[1])
                assert int(small[2]) & 0xFFFFFFFF == 0, "the sizes call: *d_err = %d" % (int(small[2]) & 0xFFFFFFFF)
                out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
                nz.batch_device(*text, out.data_ptr(), total, 0, 0, 0, small.data_ptr() + 24, stream())
                torch.cuda.synchronize()
                assert int(small[3]) & 0xFFFFFFFF == 0, "the write call: *d_err = %d" % (int(small[3]) & 0xFFFFFFFF)
                assert bool((out[total:] == 0xA5).all()), "written behind the output"
                return out[:total], oo, ch, total, changed
            out, oo, ch, total, changed = run(dev(b.data), dev(b.offs), n, b.L)  # the block alone
            assert total == TB and changed == int(ch_b.sum())
            assert np.array_equal(oo.cpu().numpy(), oo_b) and np.array_equal(ch.cpu().numpy(), ch_b)
            assert np.array_equal(out.cpu().numpy(), out_b), "the block alone differs from norm_ref"
            del out, oo, ch
            batch = Batch(b, R)
            assert batch.n_bytes >= boundary + 2 ** 26 and R * TB >= boundary + 2 ** 26
            out, oo, ch, total, changed = run(batch.bytes, batch.offs, batch.n_docs, batch.n_bytes)
            assert total == R * TB, "d_totals[0] = %d, %d copies of %d expected" % (total, R, TB)
            assert changed == R * int(ch_b.sum()), "d_totals[1] = %d, %d copies of %d expected" % (changed, R, int(ch_b.sum()))
            doc_at = lambda r, d: batch.doc_start(r, d)  # noqa: E731
            assert_offsets(oo, oo_b, R, "normalize %s, d_out_offsets" % form, doc_at)
            assert_rows(ch, dev(ch_b), R, "normalize %s, d_changed" % form, doc_at)
            assert_rows(out, dev(out_b), R, "normalize %s, text (positions in the input)" % form,
                        lambda r, j: batch.doc_start(r, int(np.searchsorted(oo_b, j, side="right")) - 1))
            del out, oo, ch, batch
    finally:
        nz.close()


# ---- 2. more than 2^31 ids ----------------------------------------------------------------------------------------------
def test_more_than_2_to_the_31_ids(oracle_mod, vg_files):
    """A block in which nearly every byte is a word, repeated until the batch holds 2^31 + 2^20 ids and more: id positions
    and out_offsets past 2^31 in the encoder, id positions past 2^31 read by the decoder."""
    import torch
    b = block("dense")
    ids_b, oo_b, st_b = oracle_rows(oracle_mod, "VG", "dense")
    assert not st_b.any() and len(ids_b) > 0.75 * b.L
    ref = DC.shipped_vocab_ref(vg_files)
    text_b, to_b = ref.decode_packed(ids_b, oo_b)
    assert np.array_equal(text_b, b.data) and np.array_equal(to_b, b.offs)
    T, n = len(ids_b), len(b.docs)
    R = W.copies_cross(T, W.B31, extra=2 ** 20)
    ctx, _files = _context("VG")
    try:
        with Row("more than 2^31 ids, VG dense", W.B31, encode_need(ctx, R * b.L, R * n) + R * b.L + 12 * R * n):
            ids, oo, st, err = encode(ctx, dev(b.data), dev(b.offs), n, b.L)  # the block alone
            assert err == 0
            assert_block_alone(b, (ids.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()), (ids_b, oo_b, st_b))
            del ids, oo, st
            batch = Batch(b, R)
            ids, oo, st, err = encode(ctx, batch.bytes, batch.offs, batch.n_docs, batch.n_bytes)
            assert err == 0
            assert int(oo[-1]) == R * T >= W.B31 + 2 ** 20

            def id_pos(r, j):
                return batch.doc_start(r, int(np.searchsorted(oo_b, j, side="right")) - 1)
            assert_offsets(oo, oo_b, R, "dense, out_offsets", lambda r, d: batch.doc_start(r, d))
            assert not st.any().item()
            assert_rows(ids[:R * T], dev(ids_b), R, "dense, ids", id_pos)
            # and back
            out = torch.full((batch.n_bytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
            boff = torch.full((batch.n_docs + 1,), -7, dtype=torch.int64, device=DEV)
            dst = torch.full((batch.n_docs,), -7, dtype=torch.int32, device=DEV)
            derr = torch.full((1,), -7, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            ctx.decode_device(ids.data_ptr(), oo.data_ptr(), batch.n_docs, R * T, out.data_ptr(), batch.n_bytes, boff.data_ptr(),
                              dst.data_ptr(), derr.data_ptr(), stream())
            torch.cuda.synchronize()
            assert int(derr.item()) == 0 and not dst.any().item()
            assert torch.equal(boff, batch.offs), "decode of more than 2^31 ids: out_offsets are not the text's offsets"
            assert_rows(out[:batch.n_bytes], dev(b.data), R, "decode of more than 2^31 ids, text", lambda r, j: r * b.L + j)
            assert bool((out[batch.n_bytes:] == 0xA5).all()), "written behind the output"
            del ids, oo, st, out, boff, dst, batch
    finally:
        ctx.close()


# ---- 6. hutk_encode_special_batch_device, hutk_encode_fallback_batch_device; 3. the decoders of their ids ---------------
_marked = {}


def special_rows(oracle_mod, vg_files):
    """The small text block with markers over it (one from p - 8 to p + 5 at each boundary, one in every third
    document) -> (bytes, where the markers are, specials_ref's ids, out_offsets, status, matches; decode_special_ref's
    text, out_offsets of those ids)"""
    if "special" not in _marked:
        b = small_block("text")
        data, at = W.marked(b)
        vp, sp, kw = vg_files
        orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
        ids, oo, st, matches = SR.encode(orc, data, b.offs, {W.EOT: W.EOT_ID})
        assert matches == len(at) > len(b.docs) // 4 and int((ids == W.EOT_ID).sum()) == matches
        ref = DC.shipped_vocab_ref(vg_files)
        specials = [(W.EOT, W.EOT_ID)]
        assert not DSR.status(ref, ids, oo, specials).any()
        text, to = DSR.decode_packed(ref, ids, oo, specials)
        _marked["special"] = (data, at, ids, oo, np.asarray(st, dtype=np.int32), matches, np.asarray(text, dtype=np.uint8),
                              np.asarray(to, dtype=np.int64))
    return _marked["special"]


def fallback_rows(oracle_mod, vl_files):
    """The small character-mode block with unknown characters over it (one with its first byte at p - 1 at each
    boundary, one in every third document) -> (bytes, table, fallback_ref's ids, out_offsets, the oracle's status;
    fallback_ref's text, out_offsets, status of those ids)"""
    if "fallback" not in _marked:
        b = small_block("chars")
        data, at = W.with_unknowns(b)
        vp, sp, kw = vl_files
        assert not kw["is_byte_encoder"]
        orc = oracle_mod.Oracle(vp, sp, kw["prefix"], False)
        table, n_lines = W.byte_table(vp)
        tt = S.TokenText(orc)
        ids, oo, st = orc.encode_packed(data, b.offs, 16)
        ids = np.asarray(ids, dtype=np.int32)
        assert int((ids == -1).sum()) >= len(at) > len(b.docs) // 8
        x_ids, x_oo, span_st = F.encode(tt, data, b.offs, ids, oo, False, table)
        assert not span_st.any() and not (x_ids == -1).any() and len(x_ids) >= len(ids) + 2 * len(at)
        text, to, dst = F.decode_packed(F.from_token_text(tt, n_lines), x_ids, x_oo, table)
        _marked["fallback"] = (data, table, x_ids, x_oo, np.asarray(st, dtype=np.int32), text, to, dst)
    return _marked["fallback"]


def _marked_encode(ctx, how, b, data, want, boundary, name, extra_per_byte, after=None):
    """Case 6 for one entry point: the block alone, then R copies, against `want` = (ids, out_offsets, status)."""
    ids_b, oo_b, st_b = want
    R = W.copies_cross(b.L, boundary)
    n, T = len(b.docs), len(ids_b)
    cap = (ctx.special_ids_capacity if how == "special" else ctx.ids_capacity)(R * b.L, R * n)
    need = encode_need(ctx, R * b.L, R * n) + extra_per_byte * R * b.L + (4 if how == "special" else 12) * cap
    with Row(name, boundary, need):
        ids, oo, st, err = encode(ctx, dev(data), dev(b.offs), n, b.L, how=how)  # the block alone
        assert err in notes(st_b)
        assert_block_alone(b, (ids.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()), (ids_b, oo_b, st_b))
        if after:
            after(1)
        del ids, oo, st
        batch = Batch(b, R, data)
        assert batch.n_bytes >= boundary + 2 ** 26
        ids, oo, st, err = encode(ctx, batch.bytes, batch.offs, batch.n_docs, batch.n_bytes, how=how)
        assert err in notes(st_b), "%s: *d_err = %d" % (name, err)
        if after:
            after(R)
        assert_offsets(oo, oo_b, R, name + ", out_offsets", lambda r, d: batch.doc_start(r, d), b.L)
        assert_rows(st, dev(st_b), R, name + ", status", lambda r, d: batch.doc_start(r, d), b.L)
        assert_rows(ids[:R * T], dev(ids_b), R, name + ", ids",
                    lambda r, j: batch.doc_start(r, int(np.searchsorted(oo_b, j, side="right")) - 1), b.L)
        del ids, oo, st, batch


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_encode_special(oracle_mod, vg_files, boundary):
    """hutk_encode_special_batch_device, VG: markers in every copy, one of them across the place where the boundary
    falls; ids, out_offsets, status and the number of matches against specials_ref."""
    b = small_block("text")
    data, at, ids_b, oo_b, st_b, matches, _text, _to = special_rows(oracle_mod, vg_files)
    p = b.p_lo if boundary == W.B31 else b.p_hi
    assert p - 8 in at and bytes(data[p - 8:p + 5]) == W.EOT
    ctx, _files = _context("VG")  # (before the memory rule: the capacities are the context's; it holds the tables only)
    try:
        ctx.set_special_tokens([(W.EOT, W.EOT_ID)])

        def count(R):
            assert ctx.special_last_matches == R * matches, "%d matches in %d copies of %d" % (ctx.special_last_matches, R, matches)
        # (the header: the special encode's workspace grows by about 2 bytes per input byte and a second id buffer)
        _marked_encode(ctx, "special", b, data, (ids_b, oo_b, st_b), boundary, "encode special VG", 2, count)
    finally:
        ctx.close()


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_encode_fallback(oracle_mod, vl_files, boundary):
    """hutk_encode_fallback_batch_device, VL: unknown characters in every copy, one of them with a byte on either side
    of the place where the boundary falls; ids, out_offsets and status against fallback_ref."""
    b = small_block("chars")
    data, table, ids_b, oo_b, st_b, _text, _to, _dst = fallback_rows(oracle_mod, vl_files)
    p = b.p_lo if boundary == W.B31 else b.p_hi
    assert bytes(data[p - 1:p + 2]) == W.UNKNOWN
    ctx, _files = _context("VL")  # (before the memory rule, as above)
    try:
        ctx.set_byte_fallback(table)
        # (the header: the fallback encode's workspace grows by 12 bytes per id the capacity allows)
        _marked_encode(ctx, "fallback", b, data, (ids_b, oo_b, st_b), boundary, "encode fallback VL", 0)
    finally:
        ctx.close()


def _marked_decode(ctx, call, want_ids, want_text, n, boundary, name):
    """Case 3 with special or byte-fallback ids: the block's ids alone, then R copies whose OUTPUT crosses the boundary;
    call(d_ids, d_id_offsets, n_docs, n_ids, d_out or 0, cap, d_out_offsets, d_status, d_err, stream)."""
    import torch
    ids_b, oo_b = want_ids
    text_b, to_b, st_b = want_text
    T, TB = len(ids_b), len(text_b)
    R = W.copies_cross(TB, boundary)
    need = 8 * R * T + 8 * (R * n + 1) + R * TB + 12 * (R * n + 1) + SCRATCH  # (ids and their renumbered copy)
    with Row(name, boundary, need):
        def run(d_ids, d_io, nd, ni, out, cap):
            oo = torch.full((nd + 1,), -7, dtype=torch.int64, device=DEV)
            st = torch.full((nd,), -7, dtype=torch.int32, device=DEV)
            err = torch.full((1,), -7, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            call(d_ids.data_ptr(), d_io.data_ptr(), nd, ni, out.data_ptr() if out is not None else 0, cap, oo.data_ptr(),
                 st.data_ptr(), err.data_ptr(), stream())
            torch.cuda.synchronize()
            return oo, st, int(err.item())
        out = torch.zeros(TB, dtype=torch.uint8, device=DEV)  # the block alone
        oo, st, err = run(dev(ids_b), dev(oo_b), n, T, out, TB)
        assert err == 0 and np.array_equal(st.cpu().numpy(), st_b) and np.array_equal(oo.cpu().numpy(), to_b)
        assert np.array_equal(out.cpu().numpy(), text_b), "the block alone differs from the reference"
        d_ids = dev(ids_b).repeat(R)
        d_io = dev(W.repeated_offsets(oo_b, T, R))
        doc_at = lambda r, d: r * TB + int(to_b[d])  # noqa: E731  (positions in the OUTPUT text)
        oo, st, err = run(d_ids, d_io, R * n, R * T, None, 0)
        assert err == 0
        assert_offsets(oo, to_b, R, name + ", the sizes call's out_offsets", doc_at, TB)
        total = int(oo[-1])
        assert total == R * TB >= boundary + 2 ** 26
        out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        oo, st, err = run(d_ids, d_io, R * n, R * T, out, total)
        assert err == 0
        assert_offsets(oo, to_b, R, name + ", out_offsets", doc_at, TB)
        assert_rows(st, dev(st_b), R, name + ", status", doc_at, TB)
        assert_rows(out[:total], dev(text_b), R, name + ", text", lambda r, j: r * TB + j, TB)
        assert bool((out[total:] == 0xA5).all()), "written behind the output"
        del out, oo, st, d_ids, d_io


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_decode_special(oracle_mod, vg_files, boundary):
    """hutk_decode_special_batch_device, VG: the ids of the special encode's reference, a marker's id in every third
    document, back to text that crosses the boundary; against decode_special_ref."""
    b = small_block("text")
    data, _at, ids_b, oo_b, _st, _m, text_b, to_b = special_rows(oracle_mod, vg_files)
    assert np.array_equal(text_b, data) and np.array_equal(to_b, b.offs)  # (byte level, no document cut: the text itself)
    ctx, _files = _context("VG")
    try:
        ctx.set_special_tokens([(W.EOT, W.EOT_ID)])
        _marked_decode(ctx, lambda i, o, nd, ni, *rest: ctx.decode_special_device(i, o, nd, ni, 0, *rest), (ids_b, oo_b),
                       (text_b, to_b, np.zeros(len(b.docs), dtype=np.int32)), len(b.docs), boundary, "decode special VG")
    finally:
        ctx.close()


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_decode_fallback(oracle_mod, vl_files, boundary):
    """hutk_decode_fallback_batch_device, VL: the ids of the fallback encode's reference, <0xHH> ids in every third
    document, back to text that crosses the boundary; against fallback_ref."""
    b = small_block("chars")
    _data, table, ids_b, oo_b, _st, text_b, to_b, dst_b = fallback_rows(oracle_mod, vl_files)
    assert np.isin(ids_b, table).sum() >= 3 * (len(b.docs) // 8)
    ctx, _files = _context("VL")
    try:
        ctx.set_byte_fallback(table)
        _marked_decode(ctx, lambda i, o, nd, ni, *rest: ctx.decode_fallback_device(i, o, nd, ni, 0, *rest), (ids_b, oo_b),
                       (text_b, to_b, dst_b), len(b.docs), boundary, "decode fallback VL")
    finally:
        ctx.close()


# ---- 7. the split presets: hutk_pretokenize_batch_device / _starts_device, the word_bits branch of k_tiles, word ids -----
_preset = {}


def split_rows(preset):
    """The small text block with the split piece over it (one from p - 9 to p + 12 at each boundary, one in every third
    document) -> (bytes, where the pieces are, presplit_ref's word starts as positions in the block, their offsets)"""
    b = small_block("text")
    if "data" not in _preset:
        _preset["data"] = W.with_split_piece(b)
    if ("starts", preset) not in _preset:
        _preset["starts", preset] = W.preset_words(_preset["data"][0], b.offs, preset)
    return _preset["data"] + _preset["starts", preset]


def preset_id_rows(oracle_mod, vg_files, preset):
    """(ids, out_offsets) of the oracle under the whole-document pattern over the restatement's words of that block"""
    if ("ids", preset) not in _preset:
        data, _at, starts, so = split_rows(preset)
        _preset["ids", preset] = W.preset_ids(oracle_mod, vg_files, data, small_block("text").offs, starts, so)
    return _preset["ids", preset]


@pytest.fixture(scope="module")
def lc_ctype():
    """the rule of tests/test_gpu_presplit.py: the whole-document pattern was checked under one LC_CTYPE"""
    import json
    import locale
    import os
    import helpers as H
    with open(os.path.join(H.GOLDEN_DIR, "g9_regex_path.json")) as f:
        want = json.load(f)["lc_ctype"]
    if locale.setlocale(locale.LC_CTYPE, None) != want:
        pytest.skip("POSIX regex matching depends on LC_CTYPE; the whole-document pattern was checked under " + want)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("preset", ["gpt2", "cl100k", "qwen2"])
def test_split_presets(preset, boundary):
    """hutoken_amd.pretokenize_packed_device (the split, the count, the listing): word starts that are byte positions past
    the boundary, a digit run, a contraction and a whitespace run around the place where it falls."""
    import torch
    import hutoken_amd
    b = small_block("text")
    data, at, starts_b, so_b = split_rows(preset)
    p = b.p_lo if boundary == W.B31 else b.p_hi
    assert p - 9 in at and bytes(data[p - 9:p + 12]) == W.SPLIT_PIECE
    n, S_ = len(b.docs), len(starts_b)
    R = W.copies_cross(b.L, boundary)
    # text and offsets, the bitmap and its prefix counts (8 bytes per 32 of text), the starts and their copy less r * L
    need = R * b.L + 16 * (R * n + 1) + R * b.L // 8 + R * b.L // 4 + 16 * R * S_ + SCRATCH
    with Row("split %s" % preset, boundary, need):
        starts, so = hutoken_amd.pretokenize_packed_device(dev(data), dev(b.offs), preset)  # the block alone
        assert np.array_equal(so.cpu().numpy(), so_b) and np.array_equal(starts.cpu().numpy(), starts_b), \
            "the block alone differs from presplit_ref (%s)" % preset
        batch = Batch(b, R, data)
        assert batch.n_bytes >= boundary + 2 ** 26
        starts, so = hutoken_amd.pretokenize_packed_device(batch.bytes, batch.offs, preset)
        what = "split %s" % preset
        assert starts.numel() == R * S_, "%s: %d word starts, %d copies of %d expected" % (what, starts.numel(), R, S_)
        rel = (starts.view(R, S_) - torch.arange(R, dtype=torch.int64, device=DEV)[:, None] * b.L).reshape(-1)
        assert_rows(rel, dev(starts_b), R, what + ", starts less r * L", lambda r, j: r * b.L + int(starts_b[j]), b.L)
        assert_offsets(so, so_b, R, what + ", start_offs", lambda r, d: batch.doc_start(r, d), b.L)
        del starts, so, rel, batch


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("preset", ["gpt2", "cl100k"])
def test_encode_under_a_preset(lc_ctype, oracle_mod, vg_files, monkeypatch, preset, boundary):
    """hutk_encode_batch_device of a context with a split preset, VG, k_tiles: the word_bits branch reads the bitmap at
    byte positions past the boundary.  Against the oracle's ids of the restatement's words."""
    monkeypatch.setenv("HUTK_PTILES", "0")
    PT = importlib.import_module("hutoken_amd.pretokenize")
    b = small_block("text")
    data, _at, _starts, _so = split_rows(preset)
    ids_b, oo_b = preset_id_rows(oracle_mod, vg_files, preset)
    n, T = len(b.docs), len(ids_b)
    st_b = np.zeros(n, dtype=np.int32)  # (the block's longest word is far below the limit: no document is cut)
    R = W.copies_cross(b.L, boundary)
    ctx, _files = _context("VG")
    try:
        ctx.set_pretokenizer(PT.preset_index(preset), PT.table_blob())
        # (the encode's need, the bitmap)
        with Row("encode VG under %s" % preset, boundary, encode_need(ctx, R * b.L, R * n) + R * b.L // 8):
            assert ctx.tile_kernel(R * b.L) == 0, "the batch would not be given the kernel this case is about"
            ids, oo, st, err = encode(ctx, dev(data), dev(b.offs), n, b.L)  # the block alone
            assert err == 0
            assert_block_alone(b, (ids.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()), (ids_b, oo_b, st_b))
            del ids, oo, st
            batch = Batch(b, R, data)
            assert batch.n_bytes >= boundary + 2 ** 26
            ids, oo, st, err = encode(ctx, batch.bytes, batch.offs, batch.n_docs, batch.n_bytes)
            what = "VG under %s" % preset
            assert err == 0, "%s: *d_err = %d" % (what, err)
            assert_offsets(oo, oo_b, R, what + ", out_offsets", lambda r, d: batch.doc_start(r, d), b.L)
            assert_rows(st, dev(st_b), R, what + ", status", lambda r, d: batch.doc_start(r, d), b.L)
            assert_rows(ids[:R * T], dev(ids_b), R, what + ", ids",
                        lambda r, j: batch.doc_start(r, int(np.searchsorted(oo_b, j, side="right")) - 1), b.L)
            del ids, oo, st, batch
    finally:
        ctx.close()


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_word_ids(vg_files, boundary):
    """hutoken_amd.token_word_ids_device under gpt2 on the batch and its own ids: the split, the count, int32 byte spans
    and the rank kernel (hutk_token_word_ids_device) at byte positions past the boundary; against features_ref.word_ids
    of the block, from spans_ref's spans of the block's ids and presplit_ref's word starts."""
    import features_ref as FR
    import hutoken_amd as hutoken
    b = small_block("text")
    data, _at, starts_b, so_b = split_rows("gpt2")
    vp, sp, _kw = vg_files
    hutoken.initialize(vp, sp, is_byte_encoder=True, pretokenizer="gpt2")
    ctx = hutoken.context()
    n = len(b.docs)
    R = W.copies_cross(b.L, boundary)
    # the encode; the spans' workspace (as in test_token_spans) and int32 spans; the bitmap, its prefix counts at 8 bytes per
    # 32 text bytes, int32 words and a status per document.  (4 ids a byte at the most: the capacity's bound)
    cap = ctx.ids_capacity(R * b.L, R * n)
    need = encode_need(ctx, R * b.L, R * n) + 5 * R * b.L + 8 * cap + R * b.L // 8 + R * b.L // 4 + 4 * cap + 4 * R * n + SCRATCH
    with Row("word ids VG gpt2", boundary, need):
        # the block alone: its ids, their spans and word ids by the restatement
        ids, oo = hutoken.encode_packed_device(dev(data), dev(b.offs), check=True)
        oo_b = oo.cpu().numpy()
        T = int(oo_b[-1])
        ids_b = ids[:T].cpu().numpy()
        tt = W.RefTokenText(DC.shipped_vocab_ref(vg_files))
        spans_b, span_st = S.batch(tt, data, b.offs, ids_b, oo_b, True, "byte", np.int64)
        assert not span_st.any() and not (ids_b == -1).any()
        words_b = np.zeros(T, dtype=np.int32)
        for d in range(n):
            rel = (starts_b[so_b[d]:so_b[d + 1]] - b.offs[d]).tolist()
            w, mismatch = FR.word_ids(None, spans_b[oo_b[d]:oo_b[d + 1]].tolist(), rel)
            assert not mismatch, d
            words_b[oo_b[d]:oo_b[d + 1]] = w
        got = hutoken.token_word_ids_device(dev(data), dev(b.offs), ids[:T], oo, check=True)
        assert np.array_equal(got.cpu().numpy(), words_b), "the block alone differs from features_ref.word_ids"
        del ids, oo, got
        batch = Batch(b, R, data)
        assert batch.n_bytes >= boundary + 2 ** 26
        ids, oo = hutoken.encode_packed_device(batch.bytes, batch.offs, check=True)

        def id_pos(r, j):
            return batch.doc_start(r, int(np.searchsorted(oo_b, j, side="right")) - 1)
        assert_offsets(oo, oo_b, R, "gpt2, out_offsets", lambda r, d: batch.doc_start(r, d), b.L)
        assert_rows(ids[:R * T], dev(ids_b), R, "gpt2, ids", id_pos, b.L)
        words = hutoken.token_word_ids_device(batch.bytes, batch.offs, ids[:R * T], oo, n_ids=R * T, check=True)
        assert words.dtype.is_signed and words.element_size() == 4
        assert_rows(words, dev(words_b), R, "word ids", id_pos, b.L)
        del ids, oo, words, batch
