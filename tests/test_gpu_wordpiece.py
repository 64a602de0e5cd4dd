"""WordPiece on the GPU (csrc/hutk_wordpiece.hip) against tests/wordpiece_ref.py, the rule restated in plain Python: id
for id, offset for offset and word id for word id, with no tolerance.  Needs a real MI355X."""
import functools

import numpy as np
import pytest

import collate_ref as CR
import pairs_ref as PR
import targets_ref as TR
import wordpiece_cases as WC
import wordpiece_ref as R

pytestmark = pytest.mark.gpu

SETTINGS = sorted(WC.SETTINGS)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _chunk():
    from hutoken_amd import _capi
    return _capi.wordpiece_chunk_bytes()


_made = {}


def _wp(lines, **opts):
    """one WordPiece per vocabulary and options (its tables are uploaded once)"""
    import hutoken_amd
    key = (tuple(lines), tuple(sorted(opts.items())))
    if key not in _made:
        _made[key] = hutoken_amd.WordPiece(list(lines), **opts)
    return _made[key]


@functools.lru_cache(maxsize=None)
def _golden_lines():
    return tuple(WC.golden_vocab())


def _ref_opts(opts):
    o = dict(opts)
    v = R.Vocab(o.pop("lines"), unk_token=o.pop("unk_token", "[UNK]"), prefix=o.pop("continuing_subword_prefix", "##"),
                max_input_chars_per_word=o.pop("max_input_chars_per_word", 100))
    return v, o


def _to_device(docs):
    import torch
    data, offs = WC.pack(docs)
    return torch.from_numpy(data).to(_dev()), torch.from_numpy(offs).to(_dev())


def _check(lines, docs, want=None, **opts):
    """encode_packed_device(return_word_ids=True) on the batch == the restatement -> the restatement's three lists"""
    wp = _wp(lines, **opts)
    if want is None:
        v, o = _ref_opts(dict(opts, lines=lines))
        want = WC.encode_docs(v, docs, **o)
    db, do = _to_device(docs)
    ids, oo, wids = wp.encode_packed_device(db, do, return_word_ids=True)
    assert ids.dtype.is_floating_point is False and str(ids.dtype) == "torch.int32" and str(oo.dtype) == "torch.int64"
    assert oo.tolist() == want[1]
    got_ids, got_w = ids.tolist(), wids.tolist()
    if got_ids != want[0] or got_w != want[2]:
        for i in range(len(docs)):
            a, b = want[1][i], want[1][i + 1]
            assert got_ids[a:b] == want[0][a:b] and got_w[a:b] == want[2][a:b], (i, docs[i][:80])
    ids2, oo2 = wp.encode_packed_device(db, do)  # (without word ids: the same ids)
    assert ids2.tolist() == want[0] and oo2.tolist() == want[1]
    return want


# ---- 1. the goldens ----
@pytest.mark.parametrize("setting", SETTINGS)
def test_goldens_through_every_entry_point(setting):
    g = WC.golden_docs()
    s = g["settings"][setting]
    opts = WC.SETTINGS[setting]
    lines = _golden_lines()
    want_ids = [t for ids in s["ids"] for t in ids]
    want_w = [t for w in s["word_ids"] for t in w]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in s["ids"]])]).tolist()
    docs = [t.encode("utf-8") for t in g["texts"]]
    _check(lines, docs, want=(want_ids, offs, want_w), **opts)
    wp = _wp(lines, **opts)
    assert wp.batch_encode(g["texts"]) == s["ids"]
    assert wp.encode(g["texts"][3]) == s["ids"][3]
    data, o = WC.pack(docs)
    ids, oo, wids = wp._handle(_dev()).batch(data, o, word_ids=True)  # the host C call
    assert ids.tolist() == want_ids and oo.tolist() == offs and wids.tolist() == want_w
    ids, oo = wp._handle(_dev()).batch(data, o)
    assert ids.tolist() == want_ids and oo.tolist() == offs
    assert wp.token_to_id("[CLS]") == 2 and wp.id_to_token(4) == "[MASK]" and wp.vocab_size == len(lines)


# ---- 2. chunk edges ----
def _edge_docs(C, shift):
    """One of each kind of thing on, one byte before and one byte after every multiple of C in the first three chunks:
    a word start, a word end, a dropped character, a two-, three- and four-byte character, a CJK character, a punctuation
    mark, a document boundary.  shift: what stands at the front, so that the fold moves the edges as well."""
    things = ["b", " ", "\u200b", "\u00e9", "\u20ac", "\U0001d49c", "\u4e2d", ",", None, "\u0130", "e\u0301"]
    batches = []
    for thing in things:
        for edge in (C, 2 * C, 3 * C):
            for delta in (-1, 0, 1):
                head = shift + "ka to "
                fill = "a" * 7 + " "
                body = head
                while len(body.encode()) + len(fill) <= edge + delta:
                    body += fill
                body += "z" * (edge + delta - len(body.encode()))
                assert len(body.encode()) == edge + delta
                tail = " mi ka,to " * 3
                if thing is None:
                    batches.append([body.encode(), tail.encode()])
                else:
                    batches.append([(body + thing + tail).encode()])
    return batches


@pytest.mark.parametrize("setting", SETTINGS)
def test_chunk_edges_in_the_source_and_in_the_folded_text(setting):
    C = _chunk()
    lines = _golden_lines()
    docs = []
    for shift in ("", "\u00e9\u0130\u200b", "\u0130\u0130\u0130 \ud55c"):
        for batch in _edge_docs(C, shift):
            docs += batch
    _check(lines, docs, **WC.SETTINGS[setting])


# ---- 3. words that go wrong ----
def test_long_words_and_trip_counts():
    lines = ("[UNK]", "a", "##a", "€", "##€")
    docs = [b"a" * 100, b"a" * 101, "€".encode() * 100, "€".encode() * 101, b"a" * 99 + b"b", b"a" * 100 + b" " + b"a" * 101,
            b"a" * (1 << 20), b" ".join([b"a"] * 4096), b".,;:!?" * 50, b"ab a b aa"]
    want = _check(lines, docs, lowercase=False)
    assert want[0][:100] == [1] + [2] * 99 and want[0][100] == 0 and want[1][5] - want[1][4] == 1
    assert want[1][7] - want[1][6] == 1 and want[1][8] - want[1][7] == 4096
    _check(("[UNK]", "a"), [b"aaa a aa"], lowercase=False)
    _check(lines, [b"a aa \xe2\x82\xac \xe2\x82\xac\xe2\x82\xac ,", b""], max_input_chars_per_word=1)
    _check(lines, [b"a aa"], max_input_chars_per_word=0)


# ---- 4. the table ----
def test_pieces_that_share_a_bucket_and_pieces_that_differ_late():
    import itertools
    base = ["[UNK]", "x", "##x"]
    probe = _wp(tuple(base), lowercase=False)._handle(_dev())
    slots = probe.info()["table_slots"]
    by_bucket = {}
    found = None
    for t in ("".join(p) for p in itertools.product("abcdefghij", repeat=3)):
        b = probe.bucket(t.encode(), False) % 16  # (a larger table keeps the low bits)
        by_bucket.setdefault(b, []).append(t)
        if len(by_bucket[b]) == 3:
            found = by_bucket[b]
            break
    assert found and slots >= 16
    one, two, three = found
    lines = tuple(base + [one, two])
    h = _wp(lines, lowercase=False)._handle(_dev())
    assert h.info()["table_slots"] == 16
    assert h.bucket(one.encode(), False) == h.bucket(two.encode(), False) == h.bucket(three.encode(), False)
    _check(lines, [("%s %s %s x%s" % (one, two, three, one)).encode()], lowercase=False)
    _check(("[UNK]",), [b"[UNK] a", b""], lowercase=False)
    _check(("a", "[UNK]", "b", "a", "##a"), [b"a b aa ab"], lowercase=False)
    long_a, long_b = "y" * 20 + "p", "y" * 20 + "q"
    _check(("[UNK]", long_a, long_b, "##" + long_b, "y", "##y"), [("%s %s %sx y%s y%s" % (long_a, long_b, long_a, long_b, long_a)).encode()],
           lowercase=False)
    _check(_golden_lines(), ["ház haz HÁZ".encode()], lowercase=False)  # the duplicated line: the later id


# ---- 5. batches ----
@pytest.mark.parametrize("docs", [[], [b""], [b""] * 5000, [b"ka"] * 5000, [b"", b" ", b"\n\n", b"\xe2\x80\x8b"]],
                         ids=["none", "one-empty", "5000-empty", "5000-one-word", "blank"])
def test_batches(docs):
    _check(_golden_lines(), docs)


# ---- 6. hostile offsets ----
@pytest.mark.parametrize("setting", ["uncased", "cased"])
def test_hostile_offsets_are_refused_and_nothing_is_written(setting):
    import torch
    from hutoken_amd import _capi
    wp = _wp(_golden_lines(), **WC.SETTINGS[setting])
    h = wp._handle(_dev())
    text = ("ka to mi, " * 30).encode()
    db = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(_dev())
    n = len(text)
    for offs in ([0, 200, 100, n], [0, 100, n + 50], [5, 100, n], [0, 100, n - 1], [0, -3, n], [0, 2**40, n], [-2**40, 0, n]):
        do = torch.tensor(offs, dtype=torch.int64, device=_dev())
        ids = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        oo = torch.full((len(offs),), -7, dtype=torch.int64, device=_dev())
        wi = torch.full((n,), -7, dtype=torch.int32, device=_dev())
        err = torch.zeros(1, dtype=torch.int32, device=_dev())
        h.batch_device(db.data_ptr(), do.data_ptr(), len(offs) - 1, n, ids.data_ptr(), n, oo.data_ptr(), wi.data_ptr(), err.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
        assert err.item() == _capi.E_ARG, offs
        assert bool((ids == -7).all()) and bool((oo == -7).all()) and bool((wi == -7).all()), offs
        with pytest.raises(ValueError):
            wp.encode_packed_device(db, do, check=True)
    _check(_golden_lines(), [text], **WC.SETTINGS[setting])  # (the handle works on)


# ---- 7. views off the 16-byte boundary ----
@pytest.mark.parametrize("off", [1, 2, 3, 5])
def test_views_off_the_16_byte_boundary(off):
    import torch
    lines = _golden_lines()
    docs = [t.encode("utf-8") for t in WC.texts(40, 21, 0, 30)]
    want = WC.encode_docs(R.Vocab(lines), docs)
    data, offs = WC.pack(docs)
    h = _wp(lines)._handle(_dev())
    n, n_docs, cap = len(data), len(docs), len(data)
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


# ---- 8. invalid UTF-8 ----
@pytest.mark.parametrize("setting", SETTINGS)
def test_invalid_utf8_at_document_ends_and_chunk_edges(setting):
    C = _chunk()
    bad = [b"\x80", b"\xbf\xbf", b"\xc3", b"\xe4\xb8", b"\xf0\x9f\x98", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xf0\x80\x80\xaf", b"\xed\xa0\x80",
           b"\xf4\x90\x80\x80", b"\xff", b"\xc3\xc3\xa9"]
    docs = []
    for b in bad:
        docs += [b, b"ka " + b, b + b" to", b"ka" + b + b"to, " + b, b"\xc3\xa9" + b]
        docs += [b"ab" + b, b"\xa9\x80 cd"]  # a sequence cut short in front of a document that starts with continuation bytes
        for delta in (-2, -1, 0, 1):
            docs.append(b"ka to " + b"a" * (C - 6 + delta) + b + b" mi")
            docs.append(b"a" * (C + delta) + b)
    _check(_golden_lines(), docs, **WC.SETTINGS[setting])


# ---- 9. one batch past 2^31 bytes ----
def test_one_batch_past_2_31_bytes():
    import torch
    lines = _golden_lines()
    docs, n = [], 0
    for t in WC.texts(6000, 77, 1, 60):
        b = t.encode("utf-8")
        if n + len(b) > (1 << 20):
            break
        docs.append(b)
        n += len(b)
    docs.append(b" " * ((1 << 20) - n))  # the block is 1 MiB of whole documents
    want = WC.encode_docs(R.Vocab(lines), docs, **WC.SETTINGS["cased"])
    data, offs = WC.pack(docs)
    reps = 2049
    block = torch.from_numpy(data).to(_dev())
    db = block.repeat(reps)
    assert db.numel() > 2**31
    base = torch.from_numpy(offs[:-1]).to(_dev())
    do = torch.cat([(base[None, :] + (torch.arange(reps, device=_dev(), dtype=torch.int64) << 20)[:, None]).reshape(-1),
                    torch.tensor([reps << 20], dtype=torch.int64, device=_dev())])
    wp = _wp(lines, **WC.SETTINGS["cased"])
    ids, oo, wids = wp.encode_packed_device(db, do, return_word_ids=True)
    per, nd = len(want[0]), len(docs)
    assert ids.numel() == per * reps and oo.dtype == torch.int64 and oo[-1].item() == per * reps
    assert ids[:per].tolist() == want[0] and wids[:per].tolist() == want[2] and oo[:nd + 1].tolist() == want[1]
    assert bool((ids.reshape(reps, per) == ids[:per][None, :]).all())
    assert bool((wids.reshape(reps, per) == wids[:per][None, :]).all())
    steps = oo[:-1].reshape(reps, nd) - (torch.arange(reps, device=_dev(), dtype=torch.int64) * per)[:, None]
    assert bool((steps == oo[:nd][None, :]).all())


# ---- 10. composition ----
def test_the_pair_goes_through_collation_packing_and_masking():
    import torch
    import hutoken_amd
    lines = _golden_lines()
    wp = _wp(lines)
    cls, sep, mask_id = wp.token_to_id("[CLS]"), wp.token_to_id("[SEP]"), wp.token_to_id("[MASK]")
    texts = WC.texts(64, 31, 0, 30)
    docs = [t.encode("utf-8") for t in texts]
    want = WC.encode_docs(R.Vocab(lines), docs)
    db, do = _to_device(docs)
    ids, oo, wids = wp.encode_packed_device(db, do, return_word_ids=True)
    h_ids, h_oo = np.array(want[0], dtype=np.int32), np.array(want[1], dtype=np.int64)
    # [CLS] A [SEP], padded
    rows, mask, lengths, plan = hutoken_amd.collate_padded(ids, oo, 48, bos_id=cls, eos_id=sep, return_plan=True)
    r = CR.padded(h_ids, h_oo, 48, bos_id=cls, eos_id=sep)
    assert np.array_equal(rows.cpu().numpy(), r[0]) and np.array_equal(mask.cpu().numpy(), r[1]) and np.array_equal(lengths.cpu().numpy(), r[2])
    # whole-word masking over the word ids
    out, labels = hutoken_amd.mask_tokens(rows, plan, mask_id=mask_id, vocab_size=wp.vocab_size, seed=9, mlm_probability=0.3,
                                          word_ids=wids, check=True)
    t = TR.mlm_ref(rows.cpu().numpy(), plan.cpu().numpy(), np.array(want[2], dtype=np.int32), seed=9, mask_id=mask_id,
                   vocab_size=wp.vocab_size, select_below=TR.threshold(0.3), mask_below=TR.threshold(0.8),
                   random_below=min(2**32, TR.threshold(0.9)))
    assert np.array_equal(out.cpu().numpy(), t[0]) and np.array_equal(labels.cpu().numpy(), t[1]) and not t[2]
    assert bool((labels != -100).any())
    # [CLS] A [SEP] B [SEP]: the first half against the second
    n = len(docs) // 2
    oo_b = oo[n:] - oo[n]
    got = hutoken_amd.collate_pairs(ids, oo[:n + 1], ids[int(oo[n].item()):], oo_b, 64, bos_id=cls, sep_ids=(sep,), eos_id=sep)
    p = PR.pairs(h_ids, h_oo[:n + 1], h_ids[h_oo[n]:], h_oo[n:] - h_oo[n], 64, bos_id=cls, sep_ids=(sep,), eos_id=sep)
    for a, b in zip(got, p):
        assert np.array_equal(a.cpu().numpy(), b)
    # packed rows
    packer = hutoken_amd.SequencePacker(32, bos_id=cls, eos_id=sep)
    ref = CR.Packer(32, bos_id=cls, eos_id=sep)
    for got_rows, ref_rows in ((packer.add(ids, oo), ref.add(h_ids, h_oo)), (packer.flush(), ref.flush())):
        for k, v in ref_rows.items():
            assert np.array_equal(got_rows[k].cpu().numpy(), v), k
