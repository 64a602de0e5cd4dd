"""A WARM word cache on every encode path, and the candidate list past its capacity.

A byte-encoder context learns from its first batch of more than 32 tiles (k_tiles lists the words its merge loop
finished, k_finish's d_learn puts them into the table of csrc/hutk_wcache.h) and reads the table in every later call: in
production a context is warm from its second batch to the end of the job.  Every case here runs three turns -- cold,
warm, warm again -- on a context with the table and on one created under HUTK_WORD_CACHE=0; both must equal the CPU
oracle (or the restatement built on it) id for id and offset for offset, every turn.  Integer work: no tolerance.

Apart from the overflow batch (20.6 MB: tests/warm_cases.py derives the size) and the batch past 2^31 bytes, every batch
is the smallest that learns, just over 32 x 960 bytes, or smaller where it must only read.  tests/test_warm_cases_cpu.py
proves what the batches claim without a GPU.  Needs a real MI355X."""
import importlib

import numpy as np
import pytest

import helpers as H
import specials_ref as SR
import view_cases as V
import warm_cases as WC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_ARG = 4
EMPTY = {"entries": 0, "appended": 0, "open": True}


def make(prefix=None, **env):
    """-> a VG context created under the environment switches `env`."""
    from hutoken_amd import _capi, data
    vp, sp, kw = data.vocab_files("VG")
    assert kw["is_byte_encoder"] and kw["prefix"] is None
    with H.env_switches(**env):
        return _capi.Context(vp, sp, prefix, True, device=0)


def oracle(prefix=None, pattern=None):
    from hutoken_amd import data
    from oracle import oracle as O
    vp, sp, _kw = data.vocab_files("VG")
    return O.Oracle(vp, sp, prefix, True, pattern=pattern)


@pytest.fixture(scope="module")
def orc():
    o = oracle()
    yield o
    o.close()


def stats(ctx):
    s = ctx.word_cache_stats()
    return {k: s[k] for k in ("entries", "appended", "open")}


def same(got, want, tag, docs=None):
    """ids and offsets of one encode against the expected ones, naming the first document that differs"""
    (ids, oo), (ids_w, oo_w) = got[:2], want[:2]
    if not np.array_equal(oo, oo_w):
        d = max(int(np.nonzero(np.asarray(oo) != np.asarray(oo_w))[0][0]) - 1, 0)
        raise AssertionError((tag, "offsets", d, None if docs is None else docs[d][:120]))
    if not np.array_equal(ids, ids_w):
        k = int(np.nonzero(np.asarray(ids) != np.asarray(ids_w))[0][0])
        d = int(np.searchsorted(oo_w, k, side="right") - 1)
        raise AssertionError((tag, "ids", d, None if docs is None else docs[d][:120], np.asarray(ids)[oo_w[d]:oo_w[d + 1]].tolist()[:40],
                              np.asarray(ids_w)[oo_w[d]:oo_w[d + 1]].tolist()[:40]))


def plain(ctx, data, offs):
    ids, oo, _st, rc = ctx.encode_packed(data, offs)
    assert rc == 0
    return ids, oo


def three_turns(ctxs, data, offs, want, tag, encode=plain, docs=None):
    """cold, warm, warm again on every context"""
    for turn in ("cold", "warm", "warm again"):
        for c, ctx in enumerate(ctxs):
            same(encode(ctx, data, offs), want, (tag, turn, "with the table" if c == 0 else "without"), docs)


def expected(orc, docs):
    data, offs = WC.pack(docs)
    ids, oo, st = orc.encode_packed(data, offs, 8)
    assert not np.asarray(st).any()
    return data, offs, (np.asarray(ids, dtype=np.int32), np.asarray(oo, dtype=np.int64))


# ---- a, b: the candidate list past its capacity ---------------------------------------------------------------------------
_over = {}


def overflow(orc):
    """The overflow batch and the oracle's ids of ALL its documents (a third of a second on the CPU: no sample is
    needed), and a small learning batch of words it does not hold; computed once for both tests."""
    if not _over:
        data, offs, starts = WC.overflow_batch()
        ids, oo, st = orc.encode_packed(data, offs, 16)
        assert not np.asarray(st).any()
        _over["big"] = (data, offs, (np.asarray(ids, dtype=np.int32), np.asarray(oo, dtype=np.int64)), len(starts))
        _over["fresh"] = expected(orc, WC.fresh_docs(3))
    return _over["big"], _over["fresh"]


def test_a_list_overflow(orc):
    """k_tiles, phase 6 (the merge loop's hand-over to the word cache): `room == false` for a wavefront whose claimed place
    is at or past wc_shard_cap; `learn_open == false` at the workgroup's start because `cnt >= wc_shard_cap`; and
    d_learn's `min(count, shard_cap)` clamp.  The statistics prove that they ran: `appended` is the sum of the clamped
    counts, so LIST_CAP means that every one of the LIST_SHARDS sub-lists was driven past its capacity.  A record written
    into the next sub-list or past the list's end would show as wrong ids in a LATER call: hence three of them and a
    fresh batch behind.  Every document of every call is compared with the oracle and with a context without the table."""
    (data, offs, want, n_words), (f_data, f_offs, f_want) = overflow(orc)
    on, off = make(), make(HUTK_WORD_CACHE="0")
    try:
        s0 = on.word_cache_stats()
        assert stats(on) == EMPTY and s0["capacity"] == 2 << 19
        same(plain(on, data, offs), want, "call 1")
        s1 = stats(on)
        print("a: after call 1", s1)
        assert s1["appended"] == WC.LIST_CAP, s1       # every sub-list clamped
        assert 0 < s1["entries"] <= s1["appended"], s1
        same(plain(on, data, offs), want, "call 2")
        s2 = stats(on)
        print("a: after call 2", s2)
        assert 0 < s2["appended"] < n_words, s2        # the words dropped in call 1 list again; those placed hit
        assert s1["entries"] <= s2["entries"] <= s0["capacity"], s2
        same(plain(on, data, offs), want, "call 3")
        s3 = stats(on)
        same(plain(off, data, offs), want, "without the table")
        same(plain(on, f_data, f_offs), f_want, "fresh words behind the overflow")
        same(plain(off, f_data, f_offs), f_want, "fresh words, without the table")
        s4 = stats(on)
        print("a: after call 3", s3, "after the fresh batch", s4)
        if s3["open"]:
            assert s4["entries"] > s3["entries"] and s4["appended"] > 0, (s3, s4)
        else:
            assert s4["entries"] == s3["entries"], (s3, s4)
        same(plain(on, data, offs), want, "call 4, behind the fresh batch")
    finally:
        on.close(), off.close()


def test_b_overflow_into_a_small_table(orc):
    """d_learn, the last workgroup's closing rule `lost > placed && lost * CLOSE_DROP_DIV >= slots` on a table of 8192 slots
    while every sub-list overflows; then k_tiles with `learn_open == false` for EVERY workgroup (the closed flag) on the
    20 MB batch, where k_finish still launches LEARN_BLOCKS workgroups of d_learn over empty sub-lists."""
    (data, offs, want, _n), (f_data, f_offs, f_want) = overflow(orc)
    ctx = make(HUTK_WORD_CACHE_LOG2="12")
    try:
        assert ctx.word_cache_stats()["capacity"] == 2 << 12 and stats(ctx) == EMPTY
        same(plain(ctx, data, offs), want, "call 1")
        s1 = ctx.word_cache_stats()
        print("b: after call 1", s1)
        assert not s1["open"] and 0 < s1["entries"] <= s1["capacity"] and s1["appended"] == WC.LIST_CAP, s1
        same(plain(ctx, data, offs), want, "call 2, closed")
        s2 = ctx.word_cache_stats()
        assert s2["entries"] == s1["entries"] and s2["appended"] == 0 and not s2["open"], s2
        same(plain(ctx, f_data, f_offs), f_want, "a small batch on the closed table")
        s3 = ctx.word_cache_stats()
        assert s3["entries"] == s1["entries"] and s3["appended"] == 0 and not s3["open"], s3
        same(plain(ctx, data, offs), want, "call 3, closed")
    finally:
        ctx.close()


# ---- c: special tokens ----------------------------------------------------------------------------------------------------
def test_c_warm_special_tokens(orc):
    """hutk_encode_special_batch_device's pieces (csrc/hutk_special.hip) through k_tiles phase 6a on a warm table: a
    piece ends a word as a document does, so a marker directly behind, in front of and between cached words leaves their
    keys as they were, a marker inside a cached word makes two other keys of it, and a marker across, on and up to a
    tile edge puts a piece's first or last word at the edge.  The piece batch has more than 32 tiles: it learns itself
    (the halves are new keys)."""
    c = WC.special_case(orc)
    on, off = make(), make(HUTK_WORD_CACHE="0")
    try:
        w_data, w_offs, w_want = expected(orc, c["warm"])
        same(plain(on, w_data, w_offs), w_want, "warming")
        e0 = stats(on)["entries"]
        assert e0 > 0
        specials = {WC.EOT: WC.EOT_ID}
        for ctx in (on, off):
            ctx.set_special_tokens(sorted(specials.items()))
        data, offs = WC.pack(c["docs"])
        ids_w, oo_w, st_w, matches = SR.encode(orc, data, offs, specials)
        assert matches >= 7 + len(c["docs"]) - 2 and not st_w.any()

        def special(ctx, d, o):
            ids, oo, st, rc = ctx.encode_special_packed(d, o)
            assert rc == 0 and not st.any() and ctx.special_last_matches == matches
            return ids, oo
        three_turns([on, off], data, offs, (ids_w, oo_w), "special", special, c["docs"])
        s = stats(on)
        assert s["entries"] > e0 and s["appended"] == 0, s  # the pieces path learned the halves; its last turn listed nothing
        same(plain(on, w_data, w_offs), w_want, "the plain batch again")  # (the plain encode never looks at the set)
    finally:
        on.close(), off.close()


# ---- d: split presets -----------------------------------------------------------------------------------------------------
def test_d_warm_split_presets():
    """k_tiles' word_bits branch with phase 6a: gpt2, cl100k and qwen2 in turn on ONE context.  A word's ids do not
    depend on the preset, so one table serves all three -- provided the key is the word's bytes as THAT preset cut them
    (wc_key with the preset's word length): a tab or full stop taken into the word, a digit run in one, in threes or in
    single digits, a contraction in either case.  Expected: the whole-pattern oracle over presplit_ref's words."""
    PT = importlib.import_module("hutoken_amd.pretokenize")
    docs = WC.preset_docs()
    data, offs = WC.pack(docs)
    whole = oracle(pattern="(.|\n)+")
    want = {p: WC.preset_expected(docs, p, whole)[:2] for p in WC.PRESETS}
    whole.close()
    assert len({w[0].tobytes() for w in want.values()}) == 3
    on, off = make(), make(HUTK_WORD_CACHE="0")
    try:
        entries = []
        for turn in ("cold", "warm", "warm again"):
            for p in WC.PRESETS:
                for c, ctx in enumerate((on, off)):
                    ctx.set_pretokenizer(PT.preset_index(p), PT.table_blob())
                    same(plain(ctx, data, offs), want[p], (p, turn, c), docs)
                entries.append(stats(on)["entries"])
        assert entries[0] > 0 and entries == sorted(entries), entries
        assert stats(on)["appended"] == 0  # the ninth call: every cacheable word of every cut is in the table
    finally:
        on.close(), off.close()


# ---- e: exception words beside hits ---------------------------------------------------------------------------------------
def test_e_exception_words_beside_hits(orc):
    """k_tiles phase 6a on a context with a prefix: every document's first word is an exception word (its record is
    written in phase 5, its bit never reaches mergem), words beyond KEY_BYTES skip the probe (`nb <= wc::KEY_BYTES`
    false) and stay pending beside lanes that hit, words of more than MAX_IDS ids are never listed (`wc::cacheable`
    false) and merge every turn; 10 to 40 pending words a tile, and one tile of more than 64, for which the `r0` loop
    takes its second trip."""
    c = WC.exception_case(orc)
    porc = oracle(prefix=WC.PREFIX)
    on, off = make(prefix=WC.PREFIX), make(prefix=WC.PREFIX, HUTK_WORD_CACHE="0")
    try:
        data, offs, want = expected(porc, c["docs"])
        three_turns([on, off], data, offs, want, "exceptions", docs=c["docs"])
        s = stats(on)
        # the table holds cached and short words only: the words beyond the key or the result were never listed
        n_cacheable = len({w for w in c["cached"] + c["short"]}) + 100  # (the padding pool's 100 words)
        assert 0 < s["entries"] <= n_cacheable, (s, n_cacheable)
    finally:
        on.close(), off.close(), porc.close()


# ---- f: two streams and the device form -----------------------------------------------------------------------------------
class Async:
    """One batch on the device; enqueue() starts hutk_encode_batch_device on a stream into fresh buffers and returns them
    WITHOUT waiting; result() waits for that stream.  A device error ends the session: nothing more is started on a GPU
    that has faulted or hung."""

    def __init__(self, ctx, data, offs):
        import torch
        self.ctx, self.n, self.nb = ctx, len(offs) - 1, int(offs[-1])
        self.db = torch.from_numpy(np.array(data, dtype=np.uint8, copy=True)).to(DEV)
        self.do = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(DEV)
        self.cap = ctx.ids_capacity(self.nb, self.n)

    def enqueue(self, stream):
        import torch
        with torch.cuda.stream(stream):  # (the fills are ordered on the stream of the call)
            ids = torch.full((self.cap,), -7, dtype=torch.int32, device=DEV)
            oo = torch.full((self.n + 1,), -7, dtype=torch.int64, device=DEV)
            err = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        try:
            self.ctx.encode_device(self.db.data_ptr(), self.do.data_ptr(), self.n, self.nb, ids.data_ptr(), self.cap,
                                   oo.data_ptr(), 0, err.data_ptr(), stream.cuda_stream)
        except RuntimeError as ex:
            pytest.exit("device failure, nothing more is run: %s" % ex, returncode=3)
        return stream, ids, oo, err

    @staticmethod
    def result(pending):
        stream, ids, oo, err = pending
        try:
            stream.synchronize()
            e = int(err.item())
        except RuntimeError as ex:
            pytest.exit("device failure, nothing more is run: %s" % ex, returncode=3)
        if e == H.E_DEVICE:
            pytest.exit("HUTK_E_DEVICE (the kernel's watchdog), nothing more is run", returncode=3)
        assert e == 0, e
        oo = oo.cpu().numpy()
        return ids[:int(oo[-1])].cpu().numpy(), oo


def test_f_two_streams_and_the_device_form(orc):
    """k_finish's d_learn on one caller stream against the next call's k_tiles (phase 6a reads the table) on ANOTHER:
    only the context's event (StreamScope: record at the end of a call, hipStreamWaitEvent at the start of the next)
    orders them.  Three calls are enqueued on streams A, B, A with no host synchronisation in between.  Then
    hutk_ctx_word_cache_clear directly behind an asynchronous call (it must wait for the event before its memsets), and
    a learning batch on B."""
    import torch
    on, off = make(), make(HUTK_WORD_CACHE="0")
    try:
        docs = WC.filler_docs(61)
        data, offs, want = expected(orc, docs)
        f_data, f_offs, f_want = expected(orc, WC.filler_docs(62))
        A, B = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        for ctx in (on, off):
            one, two = Async(ctx, data, offs), Async(ctx, f_data, f_offs)
            torch.cuda.synchronize()  # (the copies of the inputs: the only wait in front of the three calls)
            pending = [one.enqueue(A), one.enqueue(B), one.enqueue(A)]  # learns on A, hits on B, hits on A
            for k, p in enumerate(pending):
                same(Async.result(p), want, ("streams A B A", k, ctx is on), docs)
            if ctx is on:
                s = stats(on)
                assert s["entries"] > 0 and s["appended"] == 0, s  # (the third call listed nothing: the first one's words hit)
            p = two.enqueue(A)         # asynchronous: new words on their way into the table ...
            ctx.word_cache_clear()     # ... and the clear directly behind it
            if ctx is on:
                assert stats(on) == EMPTY
            q = one.enqueue(B)         # learns again, on the other stream
            same(Async.result(p), f_want, ("in front of the clear", ctx is on))
            same(Async.result(q), want, ("behind the clear", ctx is on), docs)
            if ctx is on:
                s = stats(on)
                assert s["entries"] > 0 and s["appended"] >= s["entries"], s
            same(Async.result(one.enqueue(A)), want, ("warm again behind the clear", ctx is on), docs)
    finally:
        on.close(), off.close()


# ---- g: views -------------------------------------------------------------------------------------------------------------
def test_g_views_on_a_warm_context(orc):
    """The off-boundary cases of tests/test_gpu_views.py that apply to the plain encoder -- d_ids_out one, two and three
    elements off the 16-byte boundary (k_finish's gather, element by element), and text off the boundary, which is
    refused -- on a warm context: the output's first and last ids are those of words that phase 6a takes from the
    table.  The guard zones around the ids stay untouched; a refused call leaves the table as it was."""
    import torch
    docs, first, last = WC.view_docs()
    data, offs, want = expected(orc, docs)
    k1, k2 = len(orc.encode(first)), len(orc.encode(last))
    assert want[0][:k1].tolist() == orc.encode(first) and want[0][-k2:].tolist() == orc.encode(last)
    on, off = make(), make(HUTK_WORD_CACHE="0")
    L = importlib.import_module("hutoken_amd._capi").load()
    G32 = -0x5A5A5A5B
    try:
        n, nb = len(offs) - 1, int(offs[-1])
        db = torch.from_numpy(np.array(data, copy=True)).to(DEV)
        do = torch.from_numpy(offs).to(DEV)
        assert db.data_ptr() % 16 == 0

        def call(ctx, d_bytes, shift):
            cap = ctx.ids_capacity(nb, n)
            ids, check = V.guarded(cap, shift, torch.int32, G32)
            assert (ids.data_ptr() % 16 != 0) == (shift != 0)
            oo = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
            err = torch.full((1,), -7, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            rc = L.hutk_encode_batch_device(ctx.handle, d_bytes.data_ptr(), do.data_ptr(), n, nb, ids.data_ptr(), cap, oo.data_ptr(),
                                            None, err.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            check("plain encode, ids shifted by %d" % shift)
            return rc, ids.cpu().numpy(), oo.cpu().numpy(), int(err.item())
        for ctx in (on, off):
            for turn, shift in (("cold", 1), ("warm", 2), ("warm again", 3), ("warm, aligned", 0), ("warm", 1)):
                rc, ids, oo, err = call(ctx, db, shift)
                assert rc == 0 and err == 0, (turn, shift, rc, err)
                same((ids[:len(want[0])], oo), want, (turn, shift, ctx is on), docs)
                assert (ids[len(want[0]):] == G32).all(), "written behind the last id"
            before = stats(ctx)
            bad = V.shifted(db, 1)
            assert bad.data_ptr() % 16 != 0
            rc, ids, oo, err = call(ctx, bad, 0)
            assert rc == E_ARG and (ids == G32).all() and (oo == -7).all() and err == -7
            assert stats(ctx) == before
        s = stats(on)
        assert s["entries"] > 0 and s["appended"] == 0, s
    finally:
        on.close(), off.close()


# ---- h: kernel choice -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptiles,which", [(None, 2), ("0", 0), ("1", 1)])
def test_h_kernel_choice(orc, ptiles, which):
    """Workspace::select with a table: with `which == 2` both tile kernels are enqueued and k_pre's sample of the batch
    picks one on the device; k_tiles has phases 6a and the hand-over, k_ptiles has no cache code, and k_finish's
    d_learn runs behind either (over empty sub-lists behind k_ptiles).  Latin learning batch, CJK-dense batch of learning
    size, Latin, CJK on one context; then under HUTK_PTILES=0 and =1, on contexts created under the switch.  Asserted of
    the statistics: what they can prove -- entries never fall, and a batch that listed nothing changed nothing."""
    switches = dict(HUTK_PTILES=ptiles, HUTK_PTILES_MIN_TILES="1")
    latin = expected(orc, WC.filler_docs(81))
    cjk = expected(orc, WC.cjk_docs())
    with H.env_switches(**switches):
        on, off = make(), make(HUTK_WORD_CACHE="0")
        try:
            for ctx in (on, off):
                e = [stats(ctx)["entries"]]
                for tag, (data, offs, want) in (("latin", latin), ("cjk", cjk), ("latin again", latin), ("cjk again", cjk)):
                    assert ctx.tile_kernel(int(offs[-1])) == which, "not the kernel choice this case is about"
                    ids, oo, st, err = H.DeviceBatch(ctx, data, offs).run()
                    assert err == 0 and not st.any(), (tag, err)
                    same((ids, oo), want, (tag, ptiles, ctx is on))
                    s = stats(ctx)
                    assert s["entries"] >= e[-1], (tag, s, e)
                    if s["appended"] == 0:
                        assert s["entries"] == e[-1], (tag, s, e)
                    e.append(s["entries"])
                if ctx is on and which == 0:  # k_tiles for certain: the Latin batch learned, and added nothing the second time
                    assert e[1] > 0 and e[3] == e[2], e
                if ctx is off:
                    assert e == [0] * 5
        finally:
            on.close(), off.close()


# ---- i: the one-launch form at its edges ----------------------------------------------------------------------------------
def test_i_one_launch_form_at_its_edges(orc):
    """k_tiles<..., ONE> phase 6a (hutk_encode: at most four tiles, one launch, reads the table and never learns): wc_key
    reads nine dwords at the word's first byte, bounded by the static_assert "key reads inside the window".  A cached
    word at byte 0, ending at the last byte of 4 x 960, across each of the three internal tile edges, as the only word;
    a 30-byte word with 0, 2, 3 and 5 bytes behind it, so that the key's dwords pass the text's end into the window's
    padding (make_key must mask them); inputs of exactly 2, 3, 30 and 31 bytes."""
    c = WC.one_launch_case(orc)
    w_data, w_offs, w_want = expected(orc, c["warm"])
    want = {name: orc.encode(text) for name, (text, _spans) in c["inputs"].items()}
    on, off = make(), make(HUTK_WORD_CACHE="0")
    try:
        for turn in ("cold", "warm", "warm again"):
            for ctx in (on, off):
                for name, (text, _spans) in c["inputs"].items():
                    ids, rc = ctx.encode_one(text)
                    assert rc == 0 and ids == want[name], (turn, name, ctx is on, ids[:40], want[name][:40])
                if turn == "cold":
                    assert stats(ctx)["entries"] == 0  # the one-launch form never learns
                    same(plain(ctx, w_data, w_offs), w_want, "warming")
        s = stats(on)
        assert s["entries"] > 0
    finally:
        on.close(), off.close()


# ---- j: past 2^31 bytes, warm ---------------------------------------------------------------------------------------------
def test_j_past_2_to_the_31_bytes_warm(oracle_mod, monkeypatch):
    """k_tiles phase 6a on far tiles: `tile` is int64, and a hit writes S, livem and mergem of a tile whose byte positions
    are negative as int32.  The "VG text k_tiles" case of tests/test_gpu_wide_batches.py (its block, its oracle rows,
    its memory rule) on a context warmed by the block's own words: the block alone twice (learns, then hits), then the
    copies that cross 2^31 bytes."""
    import test_gpu_wide_batches as WB
    import wide_cases as W
    monkeypatch.setenv("HUTK_PTILES", "0")
    b = WB.block("text")
    ids_b, oo_b, st_b = WB.oracle_rows(oracle_mod, "VG", "text")
    R = W.copies_cross(b.L, W.B31)
    ctx, _files = WB._context("VG")
    try:
        with WB.Row("encode VG text, warm", W.B31, WB.encode_need(ctx, R * b.L, R * len(b.docs))):
            assert ctx.tile_kernel(R * b.L) == 0, "the batch would not be given the kernel this case is about"
            for turn in ("cold", "warm"):
                ids, oo, st, err = WB.encode(ctx, WB.dev(b.data), WB.dev(b.offs), len(b.docs), b.L)
                assert err in WB.notes(st_b)
                WB.assert_block_alone(b, (ids.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()), (ids_b, oo_b, st_b))
                del ids, oo, st
            s = stats(ctx)
            assert s["entries"] > 0, s
            batch = WB.Batch(b, R)
            assert batch.n_bytes >= W.B31 + 2 ** 26
            T = len(ids_b)
            ids, oo, st, err = WB.encode(ctx, batch.bytes, batch.offs, batch.n_docs, batch.n_bytes)
            assert err in WB.notes(st_b), err
            WB.assert_offsets(oo, oo_b, R, "warm, out_offsets", lambda r, d: batch.doc_start(r, d))
            WB.assert_rows(st, WB.dev(st_b), R, "warm, status", lambda r, d: batch.doc_start(r, d))
            WB.assert_rows(ids[:R * T], WB.dev(ids_b), R, "warm, ids",
                           lambda r, j: batch.doc_start(r, int(np.searchsorted(oo_b, j, side="right")) - 1))
            assert stats(ctx)["entries"] >= s["entries"]
            del ids, oo, st, batch
    finally:
        ctx.close()
