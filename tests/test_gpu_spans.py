"""Token spans on the GPU (csrc/hutk_spans.hip) against the plain restatement of tests/spans_ref.py (pinned against the
oracle in tests/test_spans_cpu.py): every element, both units, both widths.  Needs a real MI355X."""
import random

import numpy as np
import pytest

import helpers as H
import spans_ref as S

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 4, 6


def _pair(oracle_mod, name, merges=False):
    """-> (GPU context, oracle, is_byte_encoder) of a shipped vocabulary."""
    from hutoken_amd import _capi, data
    vp, sp, kw = data.vocab_files(name)
    mp = data.merges_file(name) if merges else None
    ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0, merges_path=mp)
    orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"], merges_path=mp)
    return ctx, orc, kw["is_byte_encoder"]


def _pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in docs], out=offs[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


def _compare(ctx, tt, d, o, is_byte, tag, need_unknown=False, docs=None):
    """Encode on the GPU, then the spans of every id against the restatement: both units, both widths."""
    ids, oo, st, _rc = ctx.encode_packed(d, o)
    if need_unknown:
        assert (ids == -1).any(), tag
    for unit, code in (("byte", 0), ("char", 1)):
        want, wst = S.batch(tt, d, o, ids, oo, is_byte, unit, np.int64, docs=docs)
        assert not wst.any(), tag
        for width, dtype in ((4, np.int32), (8, np.int64)):
            got, gst, rc = ctx.token_spans_packed(d, o, ids, oo, unit=code, out_width=width)
            print("%s %s int%d: %d docs, %d ids, rc %d, mismatching documents %d" %
                  (tag, unit, 8 * width, len(o) - 1, len(ids), rc, int((gst != 0).sum())))
            assert rc == 0 and not gst.any(), (tag, unit, width)
            assert got.dtype == dtype and got.shape == (len(ids), 2)
            if docs is None:
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert bad.size == 0, (tag, unit, width, bad[:5], got[bad[:5]], want[bad[:5]])
            else:
                for i in docs:
                    a, b = int(oo[i]), int(oo[i + 1])
                    assert np.array_equal(got[a:b], want[a:b]), (tag, unit, width, i)
    return ids, oo


@pytest.mark.parametrize("name", ["VG", "VL", "VC"])
def test_shipped_vocabularies_on_the_corpora(oracle_mod, name):
    from hutoken_amd import synth
    ctx, orc, is_byte = _pair(oracle_mod, name)
    tt = S.TokenText(orc)
    for corpus, n in (("C2", 300), ("C3", 1500), ("C5", 1500)):
        d, o = synth.corpus(corpus, n)
        _compare(ctx, tt, d, o, is_byte, "%s %s" % (name, corpus), need_unknown=name == "VL" and corpus != "C5")
    rng = random.Random(5)
    d, o = _pack([H.random_text(rng, max_words=40).encode("utf-8") for _ in range(3000)])
    _compare(ctx, tt, d, o, is_byte, "%s random_text" % name, need_unknown=name == "VL")
    if is_byte:
        d, o = _pack([H.random_bytes_text(rng, rng.randint(0, 200)) for _ in range(3000)])
        _compare(ctx, tt, d, o, is_byte, "%s random_bytes_text" % name)
    ctx.close()


def test_merges_file_context(oracle_mod):
    from hutoken_amd import synth
    ctx, orc, is_byte = _pair(oracle_mod, "VG", merges=True)
    assert ctx.uses_merges
    d, o = synth.corpus("C3", 800)
    _compare(ctx, S.TokenText(orc), d, o, is_byte, "VG merges C3")
    ctx.close()


@pytest.mark.parametrize("drop", ["őű漢", "e3.", "aeiouáé字"])
def test_character_vocabulary_with_unknown_characters(tmp_path, oracle_mod, drop):
    from hutoken_amd import _capi
    ents, special = H.random_char_vocab(5, n_merges=400, drop_chars=drop)
    vp, spath = H.write_vocab(tmp_path, "c%d" % len(drop), ents, special)
    ctx, orc = _capi.Context(vp, spath, "▁", False, device=0), oracle_mod.Oracle(vp, spath, "▁", False)
    rng = random.Random(9)
    d, o = _pack([H.random_text(rng, max_words=30).encode("utf-8") for _ in range(2500)] + [b"", "é".encode(), b" ", b"  a"])
    _compare(ctx, S.TokenText(orc), d, o, False, "char vocab -%s" % drop, need_unknown=True)
    ctx.close()


def test_byte_vocabulary_with_unknown_bytes(tmp_path, oracle_mod):
    """A byte-level vocabulary that lacks some single bytes: ids of -1 that cover one byte each."""
    from hutoken_amd import _capi
    from hutoken_amd import vocab_files as vf
    ents, special = H.random_byte_vocab(3, n_merges=300)
    vis = vf.bytes_to_unicode()
    lacking = {vf.encode_visible(bytes([b]), vis) for b in (0x62, 0xC3, 0xBC, 0x80)}
    kept = [(k, i) for k, i in ents if k not in lacking]
    assert len(kept) == len(ents) - 4
    ents = kept
    vp, spath = H.write_vocab(tmp_path, "bu", ents, special)
    ctx, orc = _capi.Context(vp, spath, None, True, device=0), oracle_mod.Oracle(vp, spath, None, True)
    rng = random.Random(2)
    docs = [H.random_bytes_text(rng, rng.randint(0, 120)) for _ in range(1500)]
    docs += [H.random_text(rng, max_words=20).encode("utf-8") for _ in range(1500)]
    d, o = _pack(docs)
    _compare(ctx, S.TokenText(orc), d, o, True, "byte vocab with holes", need_unknown=True)
    ctx.close()


def _skewed_batch():
    """100 000 empty documents, a document whose ids cross several tile boundaries, short ones, more empty ones."""
    from hutoken_amd import synth
    big, _ = synth.big_document(40_000)
    small_d, small_o = synth.corpus("C3", 400)
    raw = small_d.tobytes()
    small = [raw[int(small_o[i]):int(small_o[i + 1])] for i in range(400)]
    cut = 20_011
    while (big[cut] & 0xC0) == 0x80:  # (not inside a character: the Llama-shaped context refuses invalid UTF-8)
        cut -= 1
    docs = small[:3] + [b""] * 100_000 + [big.tobytes()] + small[3:200] + [b""] * 5 + [big.tobytes()[:cut]] + small[200:] + [b"", b""]
    return _pack(docs), [0, 1, 2, 3, 50_000, 100_002, 100_003, 100_004, 100_100, 100_200, 100_201, 100_205, 100_206,
                         100_207, len(docs) - 3, len(docs) - 2, len(docs) - 1]


def test_tile_boundaries_inside_a_document_and_a_run_of_empty_documents(oracle_mod):
    ctx, orc, is_byte = _pair(oracle_mod, "VG")
    (d, o), _ = _skewed_batch()
    ids, oo = _compare(ctx, S.TokenText(orc), d, o, is_byte, "skewed VG")
    assert int(oo[100_004] - oo[100_003]) > 3 * 2048  # the long document really spans tiles
    ctx.close()
    ctx, orc, is_byte = _pair(oracle_mod, "VL")
    _compare(ctx, S.TokenText(orc), d, o, is_byte, "skewed VL")
    ctx.close()


def test_look_back_that_helps_itself(oracle_mod, monkeypatch):
    """HUTK_SPANS_HELP_AFTER=0: every tile adds an unanswered predecessor up itself at its first poll (the look-back
    must not depend on the order in which workgroups start) -- the same spans."""
    from hutoken_amd import synth
    for name in ("VG", "VL"):
        ctx, orc, is_byte = _pair(oracle_mod, name)
        big, _ = synth.big_document(3_000_000)
        d0, o0 = synth.corpus("C3", 20000)
        d = np.concatenate([d0, big])
        o = np.concatenate([o0, [len(d)]]).astype(np.int64)
        ids, oo, _st, _rc = ctx.encode_packed(d, o)
        plain = [ctx.token_spans_packed(d, o, ids, oo, unit=u, out_width=8) for u in (0, 1)]
        monkeypatch.setenv("HUTK_SPANS_HELP_AFTER", "0")
        helped = [ctx.token_spans_packed(d, o, ids, oo, unit=u, out_width=8) for u in (0, 1)]
        monkeypatch.delenv("HUTK_SPANS_HELP_AFTER")
        for (a, ast, arc), (b, bst, brc) in zip(plain, helped):
            assert arc == 0 and brc == 0 and not ast.any() and not bst.any()
            assert np.array_equal(a, b)
        last = int(oo[-1]) - 1
        assert plain[0][0][last, 1] == len(big)  # the long document's last token ends at its last byte
        tt = S.TokenText(orc)
        want, _ = S.batch(tt, d, o, ids, oo, is_byte, "byte", np.int64, docs=[0, 7, 19999])
        for i in (0, 7, 19999):
            assert np.array_equal(plain[0][0][int(oo[i]):int(oo[i + 1])], want[int(oo[i]):int(oo[i + 1])])
        ctx.close()


def test_select_by_search_gives_the_same_spans(oracle_mod, monkeypatch):
    """HUTK_SPANS_SELECT=search: character mode without the scattered select array (the form DESIGN 8b measures
    against) -- the same spans, on a batch with empty documents, ids of -1 and tile boundaries inside a document."""
    (d, o), _docs = _skewed_batch()
    ctx, _orc, is_byte = _pair(oracle_mod, "VL")
    assert not is_byte
    ids, oo, _st, _rc = ctx.encode_packed(d, o)
    assert (ids == -1).any()
    for width in (4, 8):
        for unit in (0, 1):
            plain, pst, prc = ctx.token_spans_packed(d, o, ids, oo, unit=unit, out_width=width)
            monkeypatch.setenv("HUTK_SPANS_SELECT", "search")
            got, gst, grc = ctx.token_spans_packed(d, o, ids, oo, unit=unit, out_width=width)
            monkeypatch.delenv("HUTK_SPANS_SELECT")
            assert prc == 0 and grc == 0 and not pst.any() and not gst.any()
            assert np.array_equal(got, plain), (unit, width)
    ctx.close()


def test_documents_without_ids_still_have_their_offsets_checked(vg_files):
    import torch
    import hutoken_amd
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    d_bytes = _dev(np.frombuffer(b"abc", dtype=np.uint8))
    d_ids = torch.zeros(0, dtype=torch.int32, device="cuda:0")
    zeros = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    got = hutoken_amd.token_spans_device(d_bytes, _dev(np.array([0, 2, 2, 3])), d_ids, zeros, n_ids=0)
    assert got.shape == (0, 2)
    for bad_o in ([0, 4, 4, 3], [0, 2, 1, 3], [-1, 2, 2, 3]):  # beyond the text, decreasing, negative
        with pytest.raises(TypeError, match="do not describe"):
            hutoken_amd.token_spans_device(d_bytes, _dev(np.array(bad_o)), d_ids, zeros, n_ids=0)
    with pytest.raises(TypeError, match="do not describe"):  # id offsets that do not end at n_ids
        hutoken_amd.token_spans_device(d_bytes, _dev(np.array([0, 2, 2, 3])), d_ids, _dev(np.array([0, 0, 0, 1])), n_ids=0)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def test_device_tensors_from_encode_packed_device(vg_files, oracle_mod):
    import torch
    import hutoken_amd
    from hutoken_amd import synth
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    tt = S.TokenText(oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]))
    d, o = synth.corpus("C3", 5000)
    d_bytes, d_offs = _dev(d), _dev(o)
    d_ids, d_oo = hutoken_amd.encode_packed_device(d_bytes, d_offs)
    torch.cuda.synchronize()
    oo = d_oo.cpu().numpy()
    ids = d_ids[:int(oo[-1])].cpu().numpy()
    for unit in ("byte", "char"):
        want, _ = S.batch(tt, d, o, ids, oo, True, unit, np.int64)
        for dtype in (None, torch.int32, torch.int64):
            got = hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, unit=unit, dtype=dtype)
            assert got.dtype == (torch.int64 if dtype == torch.int64 else torch.int32) and got.shape == (len(ids), 2)
            assert np.array_equal(got.cpu().numpy(), want)
    st = torch.cuda.Stream(device="cuda:0")  # asynchronous on a stream of the caller's
    with torch.cuda.stream(st):
        got = hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, unit="char", n_ids=len(ids), check=False)
    st.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_full_size_one_million_documents(vg_files, oracle_mod):
    """C3, 1 M documents x VG, the ids as encode_packed_device leaves them: invariants of every document on the device,
    a seeded sample of documents against the restatement."""
    import torch
    import hutoken_amd
    from hutoken_amd import synth
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", 1_000_000)
    d_bytes, d_offs = _dev(d), _dev(o)
    d_ids, d_oo = hutoken_amd.encode_packed_device(d_bytes, d_offs)
    torch.cuda.synchronize()
    oo = d_oo.cpu().numpy()
    n_ids = int(oo[-1])
    lens = d_offs[1:] - d_offs[:-1]
    has = d_oo[1:] > d_oo[:-1]
    tt = S.TokenText(oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]))
    sample = sorted(np.random.default_rng(11).choice(1_000_000, size=300, replace=False).tolist())
    ids = d_ids[:n_ids].cpu().numpy()
    starts = torch.zeros(len(d) + 1, dtype=torch.int64, device="cuda:0")
    torch.cumsum((d_bytes & 0xC0) != 0x80, 0, out=starts[1:])
    chars = starts[d_offs[1:]] - starts[d_offs[:-1]]  # character starts per document
    del starts
    assert bool((lens[~has] == 0).all())
    for unit in ("byte", "char"):
        spans = hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, unit=unit, n_ids=n_ids)
        last = spans[(d_oo[1:] - 1).clamp(min=0), 1].to(torch.int64)
        # every document's last token ends at its last byte, i.e. behind its last character
        assert bool((last[has] == (lens if unit == "byte" else chars)[has]).all())
        first = torch.zeros(n_ids, dtype=torch.bool, device="cuda:0")
        first[d_oo[:-1][has]] = True
        step = spans[1:, 0] >= spans[:-1, 0]
        assert bool((step | first[1:]).all())  # starts never decrease inside a document
        assert bool((spans[:, 0][first] == 0).all()) and bool((spans[:, 1] >= spans[:, 0]).all())
        want, _ = S.batch(tt, d, o, ids, oo, True, unit, np.int32, docs=sample)
        got = spans.cpu().numpy()
        for i in sample:
            assert np.array_equal(got[int(oo[i]):int(oo[i + 1])], want[int(oo[i]):int(oo[i + 1])]), (unit, i)
        del spans, got
    torch.cuda.empty_cache()


def test_one_gigabyte_document_with_int64_spans(vg_files, oracle_mod):
    """ONE document of 1 GB: the byte spans are the running sum of the tokens' lengths, the character spans follow from
    the running count of character starts -- both taken with torch on the device and compared element for element."""
    import torch
    import hutoken_amd
    from hutoken_amd import synth
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    d, o = synth.big_document(1_000_000_000)
    d_bytes, d_offs = _dev(d), _dev(o)
    d_ids, d_oo = hutoken_amd.encode_packed_device(d_bytes, d_offs)
    torch.cuda.synchronize()
    n_ids = int(d_oo[-1].item())
    assert n_ids > 100_000_000 and not bool((d_ids[:n_ids] < 0).any())
    tt = S.TokenText(oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]))
    uniq = torch.unique(d_ids[:n_ids]).cpu().tolist()
    table = np.zeros(max(uniq) + 1, dtype=np.int64)
    for i in uniq:
        table[i] = len(tt.rest(i))
    assert tt.first(int(d_ids[0].item())) == tt.rest(int(d_ids[0].item()))  # (no prefix: the first token is like the others)
    ends = torch.cumsum(_dev(table)[d_ids[:n_ids].long()], 0)
    assert int(ends[-1].item()) == len(d)
    spans = hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, unit="byte", dtype=torch.int64, n_ids=n_ids)
    assert spans.dtype == torch.int64
    assert torch.equal(spans[:, 1], ends) and torch.equal(spans[1:, 0], ends[:-1]) and int(spans[0, 0].item()) == 0
    del spans
    starts = torch.zeros(len(d) + 1, dtype=torch.int64, device="cuda:0")
    torch.cumsum((d_bytes & 0xC0) != 0x80, 0, out=starts[1:])
    spans = hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, unit="char", dtype=torch.int64, n_ids=n_ids)
    assert torch.equal(spans[:, 1], starts[ends])
    begin = torch.cat([ends.new_zeros(1), ends[:-1]])
    assert torch.equal(spans[:, 0], starts[begin + 1] - 1)  # (no token of this vocabulary is empty)
    del spans, starts, ends, begin
    torch.cuda.empty_cache()


def test_a_regex_pattern_context_is_refused(vg_files):
    from hutoken_amd import _capi
    vp, sp, kw = vg_files
    ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0)
    ctx.set_pattern("[a-z]+")
    d, o = _pack([b"some words here"])
    with pytest.raises(ValueError, match="regex pattern"):
        ctx.token_spans_packed(d, o, np.array([1, 2, 3], dtype=np.int32), np.array([0, 3], dtype=np.int64))
    ctx.close()


def test_a_tampered_id_marks_its_document_only(oracle_mod):
    from hutoken_amd import synth
    for name in ("VG", "VL"):
        ctx, orc, is_byte = _pair(oracle_mod, name)
        tt = S.TokenText(orc)
        d, o = synth.corpus("C3", 3000)
        ids, oo, _st, _rc = ctx.encode_packed(d, o)
        victim = 1234
        at = (int(oo[victim]) + int(oo[victim + 1])) // 2
        bad = ids.copy()
        for cand in range(1000, 1100):  # another token with another text
            if cand != ids[at] and tt.rest(cand) is not None and tt.rest(cand) != tt.rest(int(ids[at])):
                bad[at] = cand
                break
        assert bad[at] != ids[at]
        for unit, code in (("byte", 0), ("char", 1)):
            got, st, rc = ctx.token_spans_packed(d, o, bad, oo, unit=code, out_width=4)
            assert rc == E_UNSUPPORTED
            assert st[victim] == S.MISMATCH and int((st != 0).sum()) == 1
            others = [victim - 2, victim - 1, victim + 1, victim + 2, 0, 2999]
            want, _ = S.batch(tt, d, o, ids, oo, is_byte, unit, np.int32, docs=others)
            for i in others:
                assert np.array_equal(got[int(oo[i]):int(oo[i + 1])], want[int(oo[i]):int(oo[i + 1])]), (name, unit, i)
        # ids out of range and ids that end the text early are mismatches too, never a fault
        for value in (-2, 10 ** 7):
            bad = ids.copy()
            bad[at] = value
            _got, st, rc = ctx.token_spans_packed(d, o, bad, oo, unit=1, out_width=8)
            assert rc == E_UNSUPPORTED and st[victim] == S.MISMATCH and int((st != 0).sum()) == 1
        ctx.close()


def test_offsets_that_do_not_describe_the_buffers(vg_files):
    import torch
    import hutoken_amd
    from hutoken_amd import synth
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", 500)
    d_bytes, d_offs = _dev(d), _dev(o)
    d_ids, d_oo = hutoken_amd.encode_packed_device(d_bytes, d_offs)
    torch.cuda.synchronize()
    oo = d_oo.cpu().numpy()
    n_ids = int(oo[-1])
    with pytest.raises(TypeError, match="do not describe"):  # offsets[-1] != n_ids
        hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, n_ids=n_ids - 1)
    for which, at, value in (("ids", 0, 1), ("ids", 250, int(oo[251]) + 1), ("ids", 250, -5), ("bytes", 250, int(o[251]) + 1),
                             ("bytes", 500, int(o[500]) + 1), ("bytes", 3, -1)):
        bad_oo, bad_o = oo.copy(), o.copy()
        (bad_oo if which == "ids" else bad_o)[at] = value
        with pytest.raises(TypeError, match="do not describe"):
            hutoken_amd.token_spans_device(d_bytes, _dev(bad_o), d_ids, _dev(bad_oo), n_ids=n_ids)
    got = hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, n_ids=n_ids)  # and the context still works
    assert int(got[-1, 1].item()) > 0
    # nothing to do: no documents, or documents without ids
    empty = hutoken_amd.token_spans_device(d_bytes[:0], d_offs[:1], d_ids[:0], d_oo[:1], n_ids=0)
    assert empty.shape == (0, 2)
    zeros = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    assert hutoken_amd.token_spans_device(d_bytes[:0], zeros, d_ids[:0], zeros, n_ids=0).shape == (0, 2)


def test_a_document_of_2_to_the_31_bytes_needs_int64_spans(vg_files):
    import torch
    import hutoken_amd
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    n = 2**31 + 16
    d_bytes = torch.full((n,), 0x61, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.tensor([0, n], dtype=torch.int64, device="cuda:0")
    d_ids = torch.tensor([hutoken_amd.encode("a")[0]], dtype=torch.int32, device="cuda:0")
    d_oo = torch.tensor([0, 1], dtype=torch.int64, device="cuda:0")
    with pytest.raises(TypeError, match="int32 spans"):
        hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, dtype=torch.int32, n_ids=1)
    got = hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo, dtype=torch.int64, n_ids=1)
    assert got.cpu().tolist() == [[0, 1]]
    del d_bytes
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["VG", "VL"])
def test_python_surface(name, oracle_mod):
    import hutoken_amd
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files(name)
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    rng = random.Random(3)
    texts = [H.random_text(rng, max_words=25) for _ in range(400)] + ["", " leading space", "árvíztűrő tükörfúrógép 漢字😂"]
    ids, offsets = hutoken_amd.batch_encode_with_offsets(texts)
    assert ids == hutoken_amd.batch_encode(texts)
    unknown = 0
    for text, row, sp_row in zip(texts, ids, offsets):
        assert len(row) == len(sp_row) and all(isinstance(x, tuple) and len(x) == 2 for x in sp_row)
        parts, end = [], 0
        for (s, e) in sp_row:  # non-empty spans, without what an earlier one covered (two tokens may share a character)
            if e > s and e > end:
                parts.append(text[max(s, end):e])
                end = e
        assert "".join(parts) == text
        unknown += -1 in row
    assert (unknown > 0) == (name == "VL")
    b_ids, b_offsets = hutoken_amd.batch_encode_with_offsets(texts, unit="byte")
    assert b_ids == ids
    for text, sp_row in zip(texts, b_offsets):
        raw = text.encode("utf-8")
        assert [s for s, _e in sp_row[1:]] == [e for _s, e in sp_row[:-1]] and (not sp_row or sp_row[-1][1] == len(raw))
    one_ids, one_sp = hutoken_amd.encode_with_offsets(texts[5])
    assert one_ids == ids[5] and one_sp == offsets[5]
    with pytest.raises(ValueError, match="unit"):
        hutoken_amd.batch_encode_with_offsets(texts, unit="word")
    if name == "VG":  # check=True names the document whose ids are not its text's
        import torch
        d, o = _pack([t.encode("utf-8") for t in texts[:50]])
        d_bytes, d_offs = _dev(d), _dev(o)
        d_ids, d_oo = hutoken_amd.encode_packed_device(d_bytes, d_offs)
        torch.cuda.synchronize()
        at = int(d_oo[20].item())
        assert int(d_oo[21].item()) > at
        d_ids[at] = d_ids[at] + 1
        with pytest.raises(ValueError, match="document 20"):
            hutoken_amd.token_spans_device(d_bytes, d_offs, d_ids, d_oo)
