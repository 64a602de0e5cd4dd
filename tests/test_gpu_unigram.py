"""Unigram on the GPU (csrc/hutk_unigram.hip) against the goldens that `tokenizers` wrote and against tests/unigram_ref.py,
the rule restated in plain Python: id for id, offset for offset and word id for word id, with no tolerance.  Needs a real
MI355X."""
import functools
import itertools

import numpy as np
import pytest

import collate_ref as CR
import unigram_cases as UC
import unigram_ref as R

pytestmark = pytest.mark.gpu

SHAPES = sorted(UC.SHAPES)
M = UC.META
MB = M.encode()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _chunk():
    from hutoken_amd import _capi
    return _capi.unigram_chunk_bytes()


_made = {}


def _ug(vocab, unk_id, shape="metaspace"):
    """one Unigram per vocabulary and shape (its table is uploaded once)"""
    import hutoken_amd
    key = (tuple(vocab), unk_id, shape)
    if key not in _made:
        _made[key] = hutoken_amd.Unigram(list(vocab), unk_id, **UC.SHAPES[shape])
    return _made[key]


@pytest.fixture(scope="module", autouse=True)
def _give_the_workspaces_back():
    """A handle keeps its workspace, 14 bytes per byte of the largest batch it has seen (tens of GB after the batch past
    2^31 bytes): the handles are closed behind this file, so the files that run after it find the device's memory free."""
    yield
    for ug in _made.values():
        for h in ug._handles.values():
            h.close()
        ug._handles.clear()
    _made.clear()


@functools.lru_cache(maxsize=None)
def _golden():
    vocab, unk_id = UC.golden_vocab()
    return tuple(vocab), unk_id


def _to_device(docs):
    import torch
    data, offs = UC.pack(docs)
    return torch.from_numpy(data).to(_dev()), torch.from_numpy(offs).to(_dev())


def _check(vocab, unk_id, docs, shape="metaspace", want=None):
    """encode_packed_device(return_word_ids=True) on the batch == the restatement -> the restatement's three lists"""
    ug = _ug(vocab, unk_id, shape)
    if want is None:
        want = R.Vocab(vocab, unk_id).encode_docs(docs, **UC.SHAPES[shape])
    db, do = _to_device(docs)
    ids, oo, wids = ug.encode_packed_device(db, do, return_word_ids=True)
    assert str(ids.dtype) == "torch.int32" and str(oo.dtype) == "torch.int64" and str(wids.dtype) == "torch.int32"
    assert oo.tolist() == want[1]
    got_ids, got_w = ids.tolist(), wids.tolist()
    if got_ids != want[0] or got_w != want[2]:
        for i in range(len(docs)):
            a, b = want[1][i], want[1][i + 1]
            assert got_ids[a:b] == want[0][a:b] and got_w[a:b] == want[2][a:b], (i, docs[i][:80])
    ids2, oo2 = ug.encode_packed_device(db, do)  # (without word ids: the same ids)
    assert ids2.tolist() == want[0] and oo2.tolist() == want[1]
    return want


# ---- 1. the goldens, ids and word ids, through the four entries ----
@pytest.mark.parametrize("shape", SHAPES)
def test_goldens_through_every_entry_point(shape):
    g = UC.golden_docs()
    s = g["shapes"][shape]
    vocab, unk_id = _golden()
    want_ids = [t for ids in s["ids"] for t in ids]
    want_w = [t for w in s["word_ids"] for t in w]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in s["ids"]])]).tolist()
    docs = [t.encode("utf-8") for t in g["texts"]]
    _check(vocab, unk_id, docs, shape, want=(want_ids, offs, want_w))
    ug = _ug(vocab, unk_id, shape)
    assert ug.batch_encode(g["texts"]) == s["ids"]
    assert ug.encode(g["texts"][3]) == s["ids"][3] and ug.encode("") == []
    data, o = UC.pack(docs)
    ids, oo, wids = ug._handle(_dev()).batch(data, o, word_ids=True)  # the host C call
    assert ids.tolist() == want_ids and oo.tolist() == offs and wids.tolist() == want_w
    ids, oo = ug._handle(_dev()).batch(data, o)
    assert ids.tolist() == want_ids and oo.tolist() == offs
    assert ug.id_to_token(unk_id) == "<unk>" and ug.vocab_size == len(vocab)
    info = ug._handle(_dev()).info()
    assert info["chunk_bytes"] == _chunk() and info["vocab_size"] == len(vocab) and info["unk_id"] == unk_id and info["max_piece_bytes"] > 16


# ---- 2. chunk edges in the source and in the folded text ----
def _edge_docs(C, shift):
    """One of each kind of thing on, one byte before and one byte after the first three multiples of C: a space, a literal
    U+2581, a multi-byte character, a word start, a word end, a document boundary.  shift: what stands at the front, so that
    the fold -- a 3-byte U+2581 that becomes one byte, collapsed spaces -- moves the edges as well."""
    batches = []
    for thing in (" ", M, "é", "中", " b", "b ", None, "  ", "\t"):
        for edge in (C, 2 * C, 3 * C):
            for delta in (-1, 0, 1):
                body = shift + "ka to "
                fill = "a" * 7 + " "
                while len(body.encode()) + len(fill) <= edge + delta:
                    body += fill
                body += "z" * (edge + delta - len(body.encode()))
                assert len(body.encode()) == edge + delta
                tail = " mi ka" + M + "to " * 3
                batches.append([body.encode(), tail.encode()] if thing is None else [(body + thing + tail).encode()])
    return [d for b in batches for d in b]


@pytest.mark.parametrize("shape", SHAPES)
def test_chunk_edges_in_the_source_and_in_the_folded_text(shape):
    vocab, unk_id = _golden()
    C = _chunk()
    for shift in ("", M + "x" + M, "a   " + M + "  "):
        _check(vocab, unk_id, _edge_docs(C, shift), shape)


# ---- 3. ring and window edges ----
@pytest.mark.parametrize("longest", [15, 16, 31, 32, 63, 64, 255, 256])
def test_the_longest_key_and_the_ring(longest):
    key = ("ab" * 128)[:longest]
    vocab = (("<unk>", 0.0), ("a", -3.0), ("b", -3.0), (key, -1.0), (key[:-1], -2.5), ("c", -1.0), (M, -0.5))
    words = [key, key[:-1], key + key[-2], "c" + key, "cc" + key, key + "c" + key, key * 3, "c" * longest + key, "ba" * 200 + key]
    for shape in ("metaspace", "never_collapse"):
        _check(vocab, 0, [" ".join(words).encode()] + [w.encode() for w in words], shape)
    h = _ug(vocab, 0)._handle(_dev())
    assert h.info()["max_piece_bytes"] == longest


def test_words_of_the_groups_window():
    vocab, unk_id = _golden()
    lanes = _ug(vocab, unk_id)._handle(_dev()).info()["group_lanes"]
    docs = []
    for n in [1, 2] + [k * lanes + d for k in (1, 2, 3, 4) for d in (-1, 0, 1)]:
        docs += [("ka" * n)[:n].encode(), (" " + "é" * n)[:n + 1].encode(), ("x" * n + " " + "tö" * n).encode()]
    for shape in SHAPES:
        _check(vocab, unk_id, docs, shape)


# ---- 4. ties and paths that are not greedy ----
def test_ties_and_non_greedy_paths():
    tie = (("<unk>", 0.0), ("a", -1.0), ("aa", -2.0), ("aaa", -3.0), ("b", -1.0), ("ab", -2.0), ("ba", -2.0), ("aab", -3.0), (M, -0.25))
    docs = [b"aaa", b"aaaa", b"aaaaaaa", b"ab", b"aab", b"aba", b"baab", b"abab aaab", b"a" * 100, b"ab" * 37]
    want = _check(tie, 0, docs, "never_collapse")
    assert want[0][:3] == [3, 1, 3]  # "aaa"; "a" "aaa": of equal scores the longest last piece
    greedy = (("<unk>", 0.0), ("abc", -1.0), ("d", -9.0), ("ab", -2.0), ("cd", -2.0), ("a", -4.0), ("b", -4.0), ("c", -4.0), (M, -1.0))
    want = _check(greedy, 0, [b"abcd", b"abcdabcd abc"], "never_collapse")
    assert want[0][:2] == [3, 4]  # "ab" "cd" (-4) beats "abc" "d" (-10)
    # an unknown in the middle: the candidate exists only where no single-character line does
    hole = (("<unk>", 0.0), ("a", -1.0), ("axb", -30.0), ("b", -1.0), ("ayb", -5.0), ("y", -1.0))
    want = _check(hole, 0, [b"axb", b"ayb", b"axxb"], "never_collapse")
    assert want[0] == [2, 1, 5, 3, 1, 0, 3]  # "a" <unk> "b" scores -42 and loses to "axb" (-30); "y" has a line, so no unknown there
    vocab, unk_id = _golden()
    _check(vocab, unk_id, [b"abab ababab abababab ba ab aab", "ház házház haz".encode()])


# ---- 5. unknowns ----
def test_unknowns_fuse_inside_a_word_only():
    v = (("<unk>", -2.0), ("a", -1.0), (M + "a", -1.0), ("q", -1.0))
    docs = [b"xyz", b"xax", b"xx a xx", b"ax x", b"<unk>x", b"x<unk>", b"q<unk>q", b"<unk>", "中文".encode(), b"a\x80\x80a"]
    want = _check(v, 0, docs)
    assert want[0][:4] == [0, 0, 1, 0]      # U+2581 is unknown and fuses with "xyz": one id; then <unk> "a" <unk>, not fused
    no_meta = (("<unk>", 0.0), ("a", -1.0))  # the prefix is an unknown of its own
    for shape in SHAPES:
        want = _check(no_meta, 0, [b"ax x", b"a", b"x", b"", b" "], shape)
    assert _check(no_meta, 0, [b"ax x"])[0] == [0, 1, 0, 0]  # a word ending unknown, then a word that is all unknown: two ids
    _check((("<unk>", -1.5),), 0, [b"a b", b"", b"<unk>", b"<unk> <unk>x"])  # a vocabulary of one line
    vocab, unk_id = _golden()
    _check(vocab, unk_id, ["q<unk> <unk>q 7<unk>7 őő <unk><unk>".encode()])


# ---- 6. long words ----
def test_one_word_of_64_kib_and_4096_words_of_one_character():
    small = (("<unk>", 0.0), ("a", -1.0), ("b", -1.25), ("ab", -2.0), ("ba", -2.25), ("abab", -4.0), ("é", -1.0), ("aé", -1.75), (M, -0.5), (M + "a", -1.0))
    import random
    rng = random.Random(12)
    word = "".join(rng.choice(["a", "b", "ab", "é", "x", "abab"]) for _ in range(40000)).encode()[:64 * 1024 - 1]
    word = word[:-1] if word[-1] >= 0x80 else word
    for shape in ("metaspace", "never_collapse"):
        _check(small, 0, [b"a b", word, b"ab"], shape)
    _check(small, 0, [b" ".join([b"a", b"b", b"x", "é".encode()] * 1024), b"a b"], "whitespace_split")


def test_one_word_of_1_mib_in_closed_form():
    import torch
    vocab = (("<unk>", 0.0), ("a", -1.0), ("aa", -1.5), ("aaaa", -2.0), (M, -1.0))
    ug = _ug(vocab, 0)
    db = torch.full((1 << 20,), ord("a"), dtype=torch.uint8, device=_dev())
    do = torch.tensor([0, 1 << 20], dtype=torch.int64, device=_dev())
    ids, oo, wids = ug.encode_packed_device(db, do, return_word_ids=True)
    assert oo.tolist() == [0, 1 + (1 << 18)] and ids[0].item() == 4
    assert bool((ids[1:] == 3).all()) and bool((wids == 0).all())


# ---- 7. document shapes ----
@pytest.mark.parametrize("docs", [[], [b""], [b""] * 5000, [b"ka"] * 5000, [b"", b" ", b"  ", b"   ", b"\n\n", MB, MB + b" " + MB, b" a", b"a ", b""]],
                         ids=["none", "one-empty", "5000-empty", "5000-one-word", "blank"])
def test_batches(docs):
    vocab, unk_id = _golden()
    for shape in SHAPES:
        _check(vocab, unk_id, docs, shape)


# ---- 8. the table ----
def test_pieces_that_share_a_slot_and_the_duplicated_line():
    base = (("<unk>", 0.0), ("x", -1.0))
    probe = _ug(base, 0)._handle(_dev())
    by_bucket, found = {}, None
    for t in ("".join(p) for p in itertools.product("abcdefghij", repeat=3)):
        b = probe.bucket(t.encode()) % 16  # (a larger table keeps the low bits)
        by_bucket.setdefault(b, []).append(t)
        if len(by_bucket[b]) == 3:
            found = by_bucket[b]
            break
    assert found
    one, two, three = found
    vocab = base + ((one, -1.0), (two, -1.0))
    h = _ug(vocab, 0)._handle(_dev())
    assert h.info()["table_slots"] == 16
    assert h.bucket(one.encode()) == h.bucket(two.encode()) == h.bucket(three.encode())
    _check(vocab, 0, [("%s %s %s x%s%s" % (one, two, three, one, two)).encode()])
    long_a, long_b = "y" * 20 + "p", "y" * 20 + "q"
    _check((("<unk>", 0.0), (long_a, -1.0), (long_b, -2.0), ("y", -3.0)), 0, [("%s %s %sx y%s y%s" % (long_a, long_b, long_a, long_b, long_a)).encode()])
    dup = (("<unk>", 0.0), ("a", -9.0), ("b", -1.0), ("a", -1.0), ("ab", -1.5), ("a", -0.25))
    assert _check(dup, 0, [b"ab a"], "never_collapse")[0] == [5, 2, 0, 5]  # the last "a", with its own score


# ---- 9. hostile offsets ----
def test_hostile_offsets_are_refused_and_nothing_is_written():
    import torch
    from hutoken_amd import _capi
    vocab, unk_id = _golden()
    ug = _ug(vocab, unk_id)
    h = ug._handle(_dev())
    text = ("ka to mi " * 30).encode()
    db = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(_dev())
    n = len(text)
    for offs in ([0, 200, 100, n], [0, 100, n + 50], [5, 100, n], [0, 100, n - 1], [0, -3, n], [0, 2**40, n], [-2**40, 0, n]):
        do = torch.tensor(offs, dtype=torch.int64, device=_dev())
        cap = n + len(offs) - 1
        ids = torch.full((cap,), -7, dtype=torch.int32, device=_dev())
        oo = torch.full((len(offs),), -7, dtype=torch.int64, device=_dev())
        wi = torch.full((cap,), -7, dtype=torch.int32, device=_dev())
        err = torch.zeros(1, dtype=torch.int32, device=_dev())
        h.batch_device(db.data_ptr(), do.data_ptr(), len(offs) - 1, n, ids.data_ptr(), cap, oo.data_ptr(), wi.data_ptr(), err.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
        assert err.item() == _capi.E_ARG, offs
        assert bool((ids == -7).all()) and bool((oo == -7).all()) and bool((wi == -7).all()), offs
        with pytest.raises(ValueError):
            ug.encode_packed_device(db, do, check=True)
    # a capacity below the total: HUTK_E_CAPACITY and no id
    do = torch.tensor([0, n], dtype=torch.int64, device=_dev())
    ids = torch.full((n,), -7, dtype=torch.int32, device=_dev())
    oo = torch.full((2,), -7, dtype=torch.int64, device=_dev())
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    h.batch_device(db.data_ptr(), do.data_ptr(), 1, n, ids.data_ptr(), 5, oo.data_ptr(), 0, err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert err.item() == _capi.E_CAPACITY and bool((ids == -7).all())
    _check(vocab, unk_id, [text])  # (the handle works on)


# ---- 10. views off the 16-byte boundary ----
@pytest.mark.parametrize("off", [1, 2, 3, 5])
def test_views_off_the_16_byte_boundary(off):
    import torch
    vocab, unk_id = _golden()
    docs = [t.encode("utf-8") for t in UC.corpus(40, 21)]
    want = R.Vocab(vocab, unk_id).encode_docs(docs)
    data, offs = UC.pack(docs)
    h = _ug(vocab, unk_id)._handle(_dev())
    n, n_docs = len(data), len(docs)
    cap = n + n_docs
    store = torch.zeros(n + 64, dtype=torch.uint8, device=_dev())
    assert store.data_ptr() % 16 == 0
    store[off:off + n] = torch.from_numpy(data).to(_dev())
    do = torch.from_numpy(offs).to(_dev())
    ids_store = torch.full((cap + 16,), -7, dtype=torch.int32, device=_dev())
    w_store = torch.full((cap + 16,), -7, dtype=torch.int32, device=_dev())
    oo_store = torch.full((n_docs + 8,), -7, dtype=torch.int64, device=_dev())
    err = torch.zeros(1, dtype=torch.int32, device=_dev())
    # (int32 and int64 views can only be off by their own size: off elements)
    h.batch_device(store.data_ptr() + off, do.data_ptr(), n_docs, n, ids_store.data_ptr() + 4 * off, cap, oo_store.data_ptr() + 8,
                   w_store.data_ptr() + 4 * off, err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert err.item() == 0
    total = want[1][-1]
    assert ids_store[off:off + total].tolist() == want[0] and w_store[off:off + total].tolist() == want[2]
    assert oo_store[1:n_docs + 2].tolist() == want[1]
    assert bool((ids_store[:off] == -7).all()) and bool((ids_store[off + total:] == -7).all())
    assert bool((w_store[:off] == -7).all()) and bool((w_store[off + total:] == -7).all())
    assert oo_store[0].item() == -7 and bool((oo_store[n_docs + 2:] == -7).all())


# ---- 11. ill-formed UTF-8 (the library's own definition: a character of one byte that no piece matches) ----
@pytest.mark.parametrize("shape", SHAPES)
def test_invalid_utf8_at_document_ends_and_chunk_edges(shape):
    C = _chunk()
    bad = [b"\x80", b"\xbf\xbf", b"\xc3", b"\xe4\xb8", b"\xf0\x9f\x98", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xff",
           b"\xc3\xc3\xa9", b"\xe2\x96", b"\x96\x81", b"\xe2\x80", b"\xc2"]
    docs = []
    for b in bad:
        docs += [b, b"ka " + b, b + b" to", b"ka" + b + b"to " + b, b"\xc3\xa9" + b]
        docs += [b"ab" + b, b"\xa9\x80 cd", b"\x81 x", b"\xa0"]  # a sequence cut short in front of a document that starts with continuation bytes
        for delta in (-2, -1, 0, 1):
            docs.append(b"ka to " + b"a" * (C - 6 + delta) + b + b" mi")
            docs.append(b"a" * (C + delta) + b)
    vocab, unk_id = _golden()
    _check(vocab, unk_id, docs, shape)


# ---- 12. one batch past 2^31 bytes ----
def test_one_batch_past_2_31_bytes():
    import torch
    vocab, unk_id = _golden()
    docs, n = [], 0
    for t in UC.corpus(6000, 77):
        b = t.encode("utf-8")
        if n + len(b) > (1 << 20):
            break
        docs.append(b)
        n += len(b)
    docs.append(b"a" * ((1 << 20) - n))  # the block is 1 MiB of whole documents
    want = R.Vocab(vocab, unk_id).encode_docs(docs, **UC.SHAPES["whitespace_split"])
    data, offs = UC.pack(docs)
    reps = 2049
    block = torch.from_numpy(data).to(_dev())
    db = block.repeat(reps)
    assert db.numel() > 2**31
    base = torch.from_numpy(offs[:-1]).to(_dev())
    do = torch.cat([(base[None, :] + (torch.arange(reps, device=_dev(), dtype=torch.int64) << 20)[:, None]).reshape(-1),
                    torch.tensor([reps << 20], dtype=torch.int64, device=_dev())])
    ug = _ug(vocab, unk_id, "whitespace_split")
    ids, oo, wids = ug.encode_packed_device(db, do, return_word_ids=True)
    per, nd = len(want[0]), len(docs)
    assert ids.numel() == per * reps and oo.dtype == torch.int64 and oo[-1].item() == per * reps
    assert ids[:per].tolist() == want[0] and wids[:per].tolist() == want[2] and oo[:nd + 1].tolist() == want[1]
    assert bool((ids.reshape(reps, per) == ids[:per][None, :]).all())
    assert bool((wids.reshape(reps, per) == wids[:per][None, :]).all())
    steps = oo[:-1].reshape(reps, nd) - (torch.arange(reps, device=_dev(), dtype=torch.int64) * per)[:, None]
    assert bool((steps == oo[:nd][None, :]).all())


# ---- 13. composition ----
def test_the_pair_goes_through_collation_span_corruption_packing_and_masking():
    import torch
    import hutoken_amd
    vocab, unk_id = _golden()
    ug = _ug(vocab, unk_id, "whitespace_split")
    docs = [t.encode("utf-8") for t in UC.corpus(64, 31)]
    want = R.Vocab(vocab, unk_id).encode_docs(docs, **UC.SHAPES["whitespace_split"])
    db, do = _to_device(docs)
    ids, oo, wids = ug.encode_packed_device(db, do, return_word_ids=True)
    h_ids, h_oo = np.array(want[0], dtype=np.int32), np.array(want[1], dtype=np.int64)
    # A </s> with T5's eos_id = 1, padded
    rows, mask, lengths, plan = hutoken_amd.collate_padded(ids, oo, 48, eos_id=1, return_plan=True)
    r = CR.padded(h_ids, h_oo, 48, eos_id=1)
    assert np.array_equal(rows.cpu().numpy(), r[0]) and np.array_equal(mask.cpu().numpy(), r[1]) and np.array_equal(lengths.cpu().numpy(), r[2])
    # T5's span corruption, sentinels counting down from 32099: the rows of the uploaded reference ids give the same
    ref_rows = hutoken_amd.collate_padded(torch.from_numpy(h_ids).to(_dev()), torch.from_numpy(h_oo).to(_dev()), 48, eos_id=1, return_plan=True)
    kw = dict(sentinel_first=32099, seed=9, noise_density=0.3, target_eos_id=1, check=True)
    got = hutoken_amd.corrupt_spans(rows, mask, plan, **kw)
    ref = hutoken_amd.corrupt_spans(ref_rows[0], ref_rows[1], ref_rows[3], **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, ref)) and bool((got[0] == 32099).any()) and bool((got[2] == 32099).any())
    # whole-word masking over the word ids
    out, labels = hutoken_amd.mask_tokens(rows, plan, mask_id=2, vocab_size=ug.vocab_size, seed=9, mlm_probability=0.3, word_ids=wids, check=True)
    out2, labels2 = hutoken_amd.mask_tokens(ref_rows[0], ref_rows[3], mask_id=2, vocab_size=ug.vocab_size, seed=9, mlm_probability=0.3,
                                            word_ids=torch.tensor(want[2], dtype=torch.int32, device=_dev()), check=True)
    assert torch.equal(out, out2) and torch.equal(labels, labels2) and bool((labels != -100).any())
    # packed rows
    packer = hutoken_amd.SequencePacker(32, eos_id=1)
    ref = CR.Packer(32, eos_id=1)
    for got_rows, ref_rows in ((packer.add(ids, oo), ref.add(h_ids, h_oo)), (packer.flush(), ref.flush())):
        for k, v in ref_rows.items():
            assert np.array_equal(got_rows[k].cpu().numpy(), v), k
