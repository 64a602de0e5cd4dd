"""Byte fallback on the GPU (csrc/hutk_fallback.hip) against the plain restatement of tests/fallback_ref.py (pinned in
tests/test_fallback_cpu.py): every element of ids, offsets and status, the host form and the device form.  Needs a real
MI355X."""
import random

import numpy as np
import pytest

import decode_ref as DR
import fallback_ref as F
import helpers as H
import spans_ref as S

pytestmark = pytest.mark.gpu

E_VALUE, E_ARG, E_DEVICE, E_UNSUPPORTED, E_CAPACITY, E_INVALID_UTF8 = 2, 4, 5, 6, 7, 10
FB_SPECIAL, FB_SKIP = 1, 2
SENTINEL = -0x5A5A5A5B
TILE, REMAP_TILE = 2048, 1024


def _pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in docs], out=offs[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


def _shipped(oracle_mod, name):
    from hutoken_amd import _capi, data
    vp, sp, kw = data.vocab_files(name)
    return (_capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0),
            oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]), kw["is_byte_encoder"])


def _char_ctx(tmp_path, oracle_mod, drop, extra=()):
    """random_char_vocab(5, 400 merges) without `drop`, plus the tokens of `extra` -> (context, oracle, entries, special)"""
    from hutoken_amd import _capi
    ents, special = H.random_char_vocab(5, n_merges=400, drop_chars=drop)
    for tok in extra:
        ents.append((tok.encode("utf-8"), len(ents)))
    vp, spath = H.write_vocab(tmp_path, "fb%d" % len(drop), ents, special)
    return _capi.Context(vp, spath, "▁", False, device=0), oracle_mod.Oracle(vp, spath, "▁", False), ents, special


def _dev_encode(ctx, d, o, flags=0, cap_delta=0):
    """The device form on a stream of its own -> (ids with 8 sentinel words behind ids_cap, cap, oo, status, err, rc)."""
    import torch
    from hutoken_amd import _capi
    n, nb = len(o) - 1, int(o[-1])
    cap = (ctx.special_ids_capacity(nb, n) if flags & FB_SPECIAL else ctx.ids_capacity(nb, n)) - 1 + cap_delta
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.array(d[:nb], dtype=np.uint8, copy=True)).to(dev) if nb else torch.zeros(16, dtype=torch.uint8, device=dev)
    do = torch.from_numpy(np.asarray(o, dtype=np.int64)).to(dev)
    ids = torch.full((max(cap, 0) + 8,), SENTINEL, dtype=torch.int32, device=dev)
    oo = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    st = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    err = torch.full((1,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    rc = _capi.load().hutk_encode_fallback_batch_device(ctx.handle, db.data_ptr(), do.data_ptr(), n, nb, flags, ids.data_ptr(), cap,
                                                        oo.data_ptr(), st.data_ptr(), err.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return ids.cpu().numpy(), cap, oo.cpu().numpy(), st.cpu().numpy()[:n], int(err.item()), rc


def _check_encode(ctx, tt, d, o, is_byte, table, tag, need_unknown=True, expect_equal_plain=False):
    """Plain ids -> the restatement; the host form and the device form against it, element by element."""
    ids, oo, st, rc0 = ctx.encode_packed(d, o)
    if need_unknown:
        assert (ids == -1).any(), tag
    want, woo, mism = F.encode(tt, d, o, ids, oo, is_byte, table)
    assert not mism.any(), tag
    if expect_equal_plain:
        assert np.array_equal(want, ids) and np.array_equal(woo, oo), tag
    else:
        assert (want >= 0).all(), tag
    got, goo, gst, rc = ctx.encode_fallback_packed(d, o)
    print("%s: %d docs, %d plain ids (%d of -1) -> %d ids, rc %d" % (tag, len(o) - 1, len(ids), int((ids == -1).sum()), len(got), rc))
    assert rc == rc0 and np.array_equal(goo, woo) and np.array_equal(gst, st), tag
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, bad[:5], got[bad[:5]], want[bad[:5]])
    dids, cap, doo, dst, err, rc = _dev_encode(ctx, d, o)
    assert rc == 0 and err == rc0, (tag, rc, err)
    assert np.array_equal(doo, woo) and np.array_equal(dst, st), tag
    assert np.array_equal(dids[:len(want)], want), tag
    assert (dids[cap:] == SENTINEL).all(), "nothing is written at or beyond ids_cap"
    return want, woo


def test_shipped_llama_vocabulary(oracle_mod):
    from hutoken_amd import synth
    ctx, orc, is_byte = _shipped(oracle_mod, "VL")
    table, found = ctx.find_byte_tokens()
    assert found == 256
    ctx.set_byte_fallback(table)
    tt = S.TokenText(orc)
    for corpus, n in (("C2", 300), ("C3", 1500), ("C5", 1500)):
        d, o = synth.corpus(corpus, n)
        _check_encode(ctx, tt, d, o, is_byte, table, "VL " + corpus, need_unknown=corpus != "C5", expect_equal_plain=corpus == "C5")
    rng = random.Random(5)
    d, o = _pack([H.random_text(rng, max_words=40).encode("utf-8") for _ in range(3000)])
    _check_encode(ctx, tt, d, o, is_byte, table, "VL random_text")
    ctx.close()


def test_a_vocabulary_without_unknown_items_is_untouched(oracle_mod):
    from hutoken_amd import synth
    ctx, orc, is_byte = _shipped(oracle_mod, "VG")
    table = np.arange(100000, 100256, dtype=np.int32)  # beyond the vocabulary
    ctx.set_byte_fallback(table)
    d, o = synth.corpus("C3", 1500)
    ids, oo, st, _rc = ctx.encode_packed(d, o)
    assert not (ids == -1).any()
    got, goo, gst, _rc = ctx.encode_fallback_packed(d, o)
    assert np.array_equal(got, ids) and np.array_equal(goo, oo) and np.array_equal(gst, st)
    dids, cap, doo, dst, err, rc = _dev_encode(ctx, d, o)
    assert rc == 0 and err == 0 and np.array_equal(dids[:len(ids)], ids) and np.array_equal(doo, oo)
    ctx.close()


@pytest.mark.parametrize("drop", ["őű漢", "e3.", "aeiouáé字"])
def test_character_vocabulary_with_unknown_characters(tmp_path, oracle_mod, drop):
    ctx, orc, _ents, _special = _char_ctx(tmp_path, oracle_mod, drop)
    table, found = ctx.find_byte_tokens()
    assert found == 256
    ctx.set_byte_fallback(table)
    rng = random.Random(9)
    docs = [H.random_text(rng, max_words=30).encode("utf-8") for _ in range(2500)]
    docs += ["😂".encode(), b"", "é".encode(), b" ", "a😂😂b".encode(), "😂".encode()]
    d, o = _pack(docs)
    want, woo = _check_encode(ctx, S.TokenText(orc), d, o, False, table, "char vocab -%s" % drop)
    n = len(docs)
    emoji = want[int(woo[n - 6]):int(woo[n - 5])].tolist()  # (four bytes, not in the vocabulary)
    assert emoji[-4:] == [int(table[b]) for b in "😂".encode()]
    # Raw documents that end inside a character: a character-mode context refuses them as it always did (the plain
    # encode's HUTK_E_INVALID_UTF8), so there is no item "cut short at the document's end" to expand here; a
    # byte-encoder context takes them (test_byte_vocabulary_with_holes: random_bytes_text holds these very strings).
    for raw in (b"a\xe6\xbc", b"\xf0\x9f"):
        d, o = _pack([b"ok", raw])
        with pytest.raises(ValueError, match="UTF-8"):
            ctx.encode_packed(d, o)
        with pytest.raises(ValueError, match="UTF-8"):
            ctx.encode_fallback_packed(d, o)
        dids, cap, doo, dst, err, rc = _dev_encode(ctx, d, o)
        assert rc == 0 and err == E_INVALID_UTF8 and (dids[cap:] == SENTINEL).all()
    ctx.close()


HOLES = (0x62, 0xC3, 0xBC, 0x80)


def holes_case(tmp_path, oracle_mod):
    """-> (context, oracle, fallback table, data, offsets): a byte-level vocabulary that lacks four single bytes, on
    arbitrary bytes and on text.  (tests/test_gpu_ptiles_edges.py runs it again.)"""
    from hutoken_amd import _capi
    from hutoken_amd import vocab_files as vf
    ents, special = H.random_byte_vocab(3, n_merges=300)
    vis = vf.bytes_to_unicode()
    lacking = {vf.encode_visible(bytes([b]), vis) for b in HOLES}
    ents = [(k, i) for k, i in ents if k not in lacking]
    vp, spath = H.write_vocab(tmp_path, "fbu", ents, special)
    ctx, orc = _capi.Context(vp, spath, None, True, device=0), oracle_mod.Oracle(vp, spath, None, True)
    assert ctx.find_byte_tokens()[1] == 0
    table = np.arange(100000, 100256, dtype=np.int32)
    ctx.set_byte_fallback(table)
    rng = random.Random(2)
    docs = [H.random_bytes_text(rng, rng.randint(0, 120)) for _ in range(1500)]
    docs += [H.random_text(rng, max_words=20).encode("utf-8") for _ in range(1500)]
    d, o = _pack(docs)
    return ctx, orc, table, d, o


def test_byte_vocabulary_with_holes(tmp_path, oracle_mod):
    ctx, orc, table, d, o = holes_case(tmp_path, oracle_mod)
    want, woo = _check_encode(ctx, S.TokenText(orc), d, o, True, table, "byte vocab with holes")
    ids, oo, _st, _rc = ctx.encode_packed(d, o)
    assert np.array_equal(woo, oo), "every -1 becomes exactly one id"
    assert set(want[ids == -1].tolist()) <= {100000 + b for b in HOLES}
    ctx.close()


def test_tile_edges(tmp_path, oracle_mod):
    """Runs of empty documents, a document whose ids cross two tile boundaries and whose output crosses seven, documents
    that begin on both sides of a boundary, a -1 as the last id, trailing empty documents."""
    ctx, orc, _e, _s = _char_ctx(tmp_path, oracle_mod, "őű漢", extra=("@", "▁@"))
    table, _ = ctx.find_byte_tokens()
    ctx.set_byte_fallback(table)
    han, one = "漢".encode(), b"@"  # [▁, -1] and [▁@]
    rng = random.Random(4)
    docs = [b""] * 100_000 + [han] * 1023 + [one] + [one, one, one] + [han * 5000]
    docs += [H.random_text(rng, max_words=30).encode("utf-8") for _ in range(300)] + [b"", b"", "a漢".encode()] + [b""] * 7
    d, o = _pack(docs)
    ids, oo, _st, _rc = ctx.encode_packed(d, o)
    first = 100_000 + 1024
    assert [int(oo[first + k]) for k in range(4)] == [TILE - 1, TILE, TILE + 1, TILE + 2], "the batch is not the one this test is about"
    big = first + 3
    assert int(oo[big + 1] - oo[big]) == 5001 and (ids[int(oo[big]) + 1:int(oo[big + 1])] == -1).all()
    assert ids[-1] == -1
    want, woo = _check_encode(ctx, S.TokenText(orc), d, o, False, table, "tile edges")
    assert int(woo[big + 1] - woo[big]) == 15001 and int(woo[big + 1]) // TILE - int(woo[big]) // TILE == 7
    # only empty documents; no documents at all
    for docs in ([b""] * 5000, []):
        d, o = _pack(docs)
        got, goo, gst, rc = ctx.encode_fallback_packed(d, o)
        assert rc == 0 and len(got) == 0 and not goo.any() and len(goo) == len(docs) + 1
        dids, cap, doo, dst, err, rc = _dev_encode(ctx, d, o)
        assert rc == 0 and err == 0 and not doo.any() and not dst.any() and (dids == SENTINEL).all()
    ctx.close()


def test_capacity_one_short_is_refused_and_nothing_is_written(oracle_mod):
    ctx, _orc, _b = _shipped(oracle_mod, "VL")
    ctx.set_byte_fallback(ctx.find_byte_tokens()[0])
    d, o = _pack(["😂 é 漢字".encode()] * 40)
    for flags in (0, FB_SPECIAL):
        dids, cap, doo, dst, err, rc = _dev_encode(ctx, d, o, flags, cap_delta=-1)
        assert rc == E_CAPACITY and (dids == SENTINEL).all() and (doo == -7).all() and err == -7
        dids, cap, doo, dst, err, rc = _dev_encode(ctx, d, o, flags)
        assert rc == 0 and err == 0 and (dids[cap:] == SENTINEL).all() and (dids[:int(doo[-1])] >= 0).all()
    ctx.close()


SPECIALS = {b"<|endoftext|>": 32000, b"<|im_start|>": 32001, b"<s>": 1}


def test_with_special_tokens(oracle_mod):
    ctx, orc, is_byte = _shipped(oracle_mod, "VL")
    table, _ = ctx.find_byte_tokens()
    ctx.set_special_tokens(list(SPECIALS.items()))
    rng = random.Random(12)
    marks = [m.decode() for m in SPECIALS]
    texts = ["<s>😂<|endoftext|>", "😂<s>漢", "<|im_start|>user\nő😂<|endoftext|>", "<s>", "😂", "", "<s><s>", "a<|endoftext|>"]
    for _ in range(400):
        t = H.random_text(rng, max_words=12)
        cut = rng.randint(0, len(t))
        texts.append(rng.choice(marks + [""]) + t[:cut] + rng.choice(marks) + "😂" + t[cut:] + rng.choice(marks + [""]))
    d, o = _pack([t.encode("utf-8") for t in texts])
    before = ctx.encode_special_packed(d, o)
    ctx.set_byte_fallback(table)
    after = ctx.encode_special_packed(d, o)
    for a, b in zip(before[:3], after[:3]):
        assert np.array_equal(a, b), "the special encode never looks at the table"
    assert (before[0] == -1).any()
    want, woo, wst = F.encode_special(orc, S.TokenText(orc), d, o, SPECIALS, is_byte, table)
    assert (want >= 0).all()
    got, goo, gst, rc = ctx.encode_fallback_packed(d, o, FB_SPECIAL)
    assert rc == 0 and np.array_equal(goo, woo) and np.array_equal(gst, wst) and np.array_equal(got, want)
    dids, cap, doo, dst, err, rc = _dev_encode(ctx, d, o, FB_SPECIAL)
    assert rc == 0 and err == 0 and np.array_equal(doo, woo) and np.array_equal(dids[:len(want)], want)
    assert (dids[cap:] == SENTINEL).all()
    # without the flag the markers are text
    plain = ctx.encode_fallback_packed(d, o)[0]
    assert not np.isin(plain, [32000, 32001]).any()
    ctx.close()


def _dev_decode(ctx, ids, offs, flags, shift=0, cap_delta=0, sizes_only=False):
    """The device form -> (bytes written, 8 guard bytes behind bytes_cap, out_offsets, status, err, rc); the output
    starts `shift` bytes into its tensor."""
    import torch
    from hutoken_amd import _capi
    dev = torch.device("cuda", 0)
    n = len(offs) - 1
    di = torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(dev)
    do = torch.from_numpy(np.asarray(offs, dtype=np.int64)).to(dev)
    oo = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    st = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    err = torch.full((1,), -7, dtype=torch.int32, device=dev)
    L = _capi.load()
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    rc = L.hutk_decode_fallback_batch_device(ctx.handle, di.data_ptr() if len(ids) else None, do.data_ptr(), n, len(ids), flags,
                                             None, 0, oo.data_ptr(), st.data_ptr(), err.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    if rc or sizes_only:
        return None, None, oo.cpu().numpy(), st.cpu().numpy()[:n], int(err.item()), rc
    total = int(oo[-1].item())
    cap = total + cap_delta
    out = torch.full((shift + max(cap, 0) + 8,), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = L.hutk_decode_fallback_batch_device(ctx.handle, di.data_ptr() if len(ids) else None, do.data_ptr(), n, len(ids), flags,
                                             out.data_ptr() + shift, cap, oo.data_ptr(), st.data_ptr(), err.data_ptr(),
                                             stream.cuda_stream)
    stream.synchronize()
    raw = out.cpu().numpy()
    return raw[shift:shift + max(cap, 0)], raw[shift + max(cap, 0):], oo.cpu().numpy(), st.cpu().numpy()[:n], int(err.item()), rc


def _check_decode(ctx, tokens, ids, offs, table, specials, tag, all_flags=False):
    """all_flags: the special flags are checked without a set too (they then change nothing)."""
    ids = np.asarray(ids, dtype=np.int32)
    offs = np.asarray(offs, dtype=np.int64)
    for flags, sp, skip in ((0, None, False), (FB_SPECIAL, specials, False), (FB_SPECIAL | FB_SKIP, specials, True)):
        if flags and not specials and not all_flags:
            continue
        want, woo, wst = F.decode_packed(tokens, ids, offs, table, sp, skip)
        if wst.any():
            with pytest.raises((ValueError, RuntimeError)):
                ctx.decode_fallback_packed(ids, offs, flags)
        else:
            got, goo, gst = ctx.decode_fallback_packed(ids, offs, flags)
            assert np.array_equal(goo, woo) and got.tobytes() == want.tobytes() and not gst.any(), (tag, flags)
        for shift in (0, 3):
            out, guard, doo, dst, err, rc = _dev_decode(ctx, ids, offs, flags, shift=shift)
            assert rc == 0 and np.array_equal(doo, woo) and np.array_equal(dst, wst), (tag, flags, shift)
            assert err in ((E_VALUE, E_UNSUPPORTED) if wst.any() else (0,)), (tag, flags)
            assert out.tobytes() == want.tobytes() and (guard == 0xEE).all(), (tag, flags, shift)
        _o, _g, doo, dst, err, rc = _dev_decode(ctx, ids, offs, flags, sizes_only=True)
        assert rc == 0 and np.array_equal(doo, woo) and np.array_equal(dst, wst), (tag, flags, "sizes only")
        if woo[-1] > 0:
            out, guard, doo, dst, err, rc = _dev_decode(ctx, ids, offs, flags, cap_delta=-1)
            assert rc == 0 and (guard == 0xEE).all() and np.array_equal(doo, woo), (tag, flags, "one short")
            assert err == E_CAPACITY or (wst.any() and err in (E_VALUE, E_UNSUPPORTED)), (tag, flags, "one short")  # (the first error stays)


@pytest.mark.parametrize("lines", [True, False])
def test_decode(tmp_path, oracle_mod, lines):
    """A prefix vocabulary; the table's ids are the vocabulary's lines (whose own text is "<0xHH>") or no lines at all."""
    ctx, orc, ents, special = _char_ctx(tmp_path, oracle_mod, "őű漢")
    ref = DR.DecodeRef(ents, special, "▁", False)
    tokens = F.from_decode_ref(ref)
    table = ctx.find_byte_tokens()[0] if lines else np.arange(100000, 100256, dtype=np.int32)
    ctx.set_byte_fallback(table)
    specials = [(b"<|eot|>", len(ents) + 5), (b"<s>", 300)]
    ctx.set_special_tokens(specials)
    fb = lambda s: [int(table[b]) for b in s.encode("utf-8")]
    pre = next(i for k, i in ents if k.decode().startswith("▁") and len(k.decode()) > 1)  # a token that starts with the prefix
    eot, bos = specials[0][1], specials[1][1]
    docs = [fb("é") + [pre, pre], [pre] + fb("漢"), fb("ő"), [pre, pre], [], fb("😂") + [eot] + fb("a") + [pre], [bos, pre, eot, pre] + fb("ű"),
            [bos] + fb("é") + [pre], [eot, bos, pre], [bos, eot], [pre] + fb("é") + [eot, bos, pre, pre], []]
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in docs], out=offs[1:])
    flat = [i for x in docs for i in x]
    _check_decode(ctx, tokens, flat, offs, table, specials, "by hand")
    got, _oo, _st = ctx.decode_fallback_packed(np.asarray(docs[0], np.int32), np.array([0, len(docs[0])]))
    assert got.tobytes()[:2] == "é".encode() and got.tobytes()[2:3] == b" ", "the token behind a fallback id keeps its prefix"
    # a bad id beside fallback ids marks its document and contributes nothing
    bad = len(ents) + 17 if lines else 100300
    _check_decode(ctx, tokens, fb("é") + [bad] + fb("a") + [pre], [0, 4, 6], table, specials, "bad id")
    # long batches: the decode tile (2048 ids) and the pass's tile (1024 ids) inside documents
    rng = random.Random(21)
    pool = [i for _k, i in ents[256:]] + [int(t) for t in table] * 2 + [eot, bos] * 20
    lens = [REMAP_TILE - 1, 1, 1, REMAP_TILE + 1, TILE - 1, 0, 0, 3 * TILE + 5, 7]
    flat = [rng.choice(pool) for _ in range(sum(lens))]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    _check_decode(ctx, tokens, flat, offs, table, specials, "long")
    # an id that is both special and in the table is refused with the special flag only
    ctx.set_special_tokens([(b"<x>", int(table[65]))])
    from hutoken_amd import _capi
    with pytest.raises(ValueError, match="both"):
        ctx.decode_fallback_packed(np.array([pre], np.int32), np.array([0, 1]), FB_SPECIAL)
    ctx.decode_fallback_packed(np.array([pre], np.int32), np.array([0, 1]), 0)
    d, o = _pack([b"a<x>"])
    with pytest.raises(ValueError, match="both"):
        ctx.encode_fallback_packed(d, o, FB_SPECIAL)
    assert _dev_encode(ctx, d, o, FB_SPECIAL)[5] == E_VALUE and _dev_encode(ctx, d, o, 0)[5] == 0
    ctx.close()


FLAG_FORMS = ((0, False), (FB_SPECIAL, False), (FB_SPECIAL | FB_SKIP, True))
ORDER_LENS = [REMAP_TILE - 1, 1, REMAP_TILE + 1, TILE - 1, 0, TILE + 5]  # both passes' tile edges inside documents


def _order_batches(seed, ents, table, eot, bos, pre):
    """The twelve documents of test_decode and one long batch, for a table and two ids that are special where a set is
    installed -> [(tag, ids, offsets)]"""
    fb = lambda s: [int(table[b]) for b in s.encode("utf-8")]
    docs = [fb("é") + [pre, pre], [pre] + fb("漢"), fb("ő"), [pre, pre], [], fb("😂") + [eot] + fb("a") + [pre], [bos, pre, eot, pre] + fb("ű"),
            [bos] + fb("é") + [pre], [eot, bos, pre], [bos, eot], [pre] + fb("é") + [eot, bos, pre, pre], []]
    rng = random.Random(seed)
    pool = [i for _k, i in ents[256:]] + [int(t) for t in table] * 2 + [eot, bos] * 20
    out = []
    for tag, rows in (("by hand", docs), ("long", [[rng.choice(pool) for _ in range(n)] for n in ORDER_LENS])):
        offs = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in rows], out=offs[1:])
        out.append((tag, np.asarray([i for x in rows for i in x], dtype=np.int32), offs))
    return out


def _order_expected(tokens, batches, table, specials):
    """What the reference gives for the batches with this table and this set (None: none) installed, every flag form."""
    return [(raw.tobytes(), oo.tolist())
            for _tag, ids, offs in batches for flags, skip in FLAG_FORMS
            for raw, oo, _st in [F.decode_packed(tokens, ids, offs, table, specials if flags else None, skip)]]


def order_plan(ents, special, prefix, is_byte):
    """The states test_decode_tables_through_every_order_of_installation walks a context through, from the references
    alone -> (tokens of fallback_ref, DecodeRef, states); a state is a dict of name, table, specials (None: no set), batches
    (for the fallback decode) and special_batches (ids of vocabulary lines only: for the special decode).  Asserts what
    catches a stale table: with the tables of the state before it, some document of a state would decode otherwise."""
    ref = DR.DecodeRef(ents, special, prefix, is_byte)
    tokens = F.from_decode_ref(ref)
    by_key = {k: i for k, i in ents}
    if all(("<0x%02X>" % b).encode() in by_key for b in range(256)):
        lines = np.array([by_key[("<0x%02X>" % b).encode()] for b in range(256)], dtype=np.int32)
    else:  # (no such lines: the last 256 lines, whatever their text)
        lines = np.arange(len(ents) - 256, len(ents), dtype=np.int32)
    other = np.arange(100000, 100256, dtype=np.int32)
    free = [i for k, i in ents[256:] if i not in set(lines.tolist())]  # lines that are in no table
    pre = next((i for k, i in ents if i in free and prefix and k.decode().startswith(prefix) and len(k.decode()) > 1), free[5])
    line_a, line_b, o1, o2 = free[10], free[11], free[12], free[13]
    assert len({pre, line_a, line_b, o1, o2}) == 5
    n = len(ents)
    set_a = [(b"<|eot|>", n + 5), (b"<|im_start|>", line_a)]  # 7 bytes: inline; 12: in the blob
    set_b = [(b"<b>", n + 9), (b"<|extends-the-blob|>", line_b), (b"<never-decoded>", n + 9)]  # two strings, one id
    states = []
    for k, (name, table, specials, eot, bos) in enumerate((
            ("1 table only", lines, None, o1, o2), ("2 plus set A", lines, set_a, n + 5, line_a),
            ("3 set B for set A", lines, set_b, n + 9, line_b), ("4 a refused set", lines, set_b, n + 9, line_b),
            ("5 set removed", lines, None, line_b, o2), ("6 set A, then the table", lines, set_a, n + 5, line_a),
            ("7 another table", other, set_a, n + 5, line_a))):
        seed = 3 if k == 3 else k  # (state 4 asks state 3's questions again)
        states.append(dict(name=name, table=table, specials=specials, batches=_order_batches(seed, ents, table, eot, bos, pre),
                           special_batches=_order_batches(seed, ents, lines, eot, bos, pre)))
    for prev, cur in zip(states, states[1:]):
        mine = _order_expected(tokens, cur["batches"], cur["table"], cur["specials"])
        stale = _order_expected(tokens, cur["batches"], prev["table"], prev["specials"])
        assert (mine == stale) == (cur["name"][0] == "4"), "stale tables would go unnoticed: " + cur["name"]
    return tokens, ref, states


def _check_decode_special(ctx, ref, state):
    import decode_special_ref as DSR
    for tag, ids, offs in state["special_batches"]:
        for flags, skip in ((0, False), (1, True)):  # HUTK_DECODE_SKIP_SPECIAL
            want, woo = DSR.decode_packed(ref, ids, offs, state["specials"], skip)
            assert not DSR.status(ref, ids, offs, state["specials"]).any()
            got, goo, gst = ctx.decode_special_packed(ids, offs, flags)
            assert np.array_equal(goo, woo) and got.tobytes() == want.tobytes() and not gst.any(), (state["name"], tag, flags)


def _check_order_encode(ctx, orc, is_byte, state):
    texts = ["<|eot|>😂<|im_start|>", "😂<|eot|>漢", "<|im_start|>", "", "a<|eot|>b", "<|im_start|><|eot|>é"]
    d, o = _pack([t.encode("utf-8") for t in texts])
    want, woo, wst = F.encode_special(orc, S.TokenText(orc), d, o, dict(state["specials"]), is_byte, state["table"])
    got, goo, gst, rc = ctx.encode_fallback_packed(d, o, FB_SPECIAL)
    assert rc == 0 and np.array_equal(goo, woo) and np.array_equal(gst, wst) and np.array_equal(got, want), state["name"]
    assert (want >= 0).all() and np.isin([i for _s, i in state["specials"]], want).all(), state["name"]


def order_vocab(kind):
    """-> (entries, special, prefix, is_byte_encoder) of the two vocabularies of the test below"""
    if kind == "char":
        return (*H.random_char_vocab(5, n_merges=400, drop_chars="őű漢"), "▁", False)
    return (*H.random_byte_vocab(3, n_merges=300), None, True)


@pytest.mark.parametrize("kind", ["char", "byte"])
def test_decode_tables_through_every_order_of_installation(tmp_path, oracle_mod, kind):
    """One context through: table; + set A; set B for A; a refused set; no set; no table, set A, the table again; another
    table.  The decode tables of the set and of the table are rebuilt from one another at every step; in every state both
    decodes must give what the references give, and order_plan has checked that the tables of the state before would not."""
    from hutoken_amd import _capi
    ents, special, prefix, is_byte = order_vocab(kind)
    vp, spath = H.write_vocab(tmp_path, "order_" + kind, ents, special)
    ctx, orc = _capi.Context(vp, spath, prefix, is_byte, device=0), oracle_mod.Oracle(vp, spath, prefix, is_byte)
    tokens, ref, states = order_plan(ents, special, prefix, is_byte)

    def check(state):
        for tag, ids, offs in state["batches"]:
            _check_decode(ctx, tokens, ids, offs, state["table"], state["specials"], state["name"] + ", " + tag, all_flags=True)
        if state["specials"]:
            _check_decode_special(ctx, ref, state)
    ctx.set_byte_fallback(states[0]["table"])
    check(states[0])
    ctx.set_special_tokens(states[1]["specials"])
    check(states[1])
    _check_order_encode(ctx, orc, is_byte, states[1])
    ctx.set_special_tokens(states[2]["specials"])
    check(states[2])
    with pytest.raises(ValueError, match="equal"):
        ctx.set_special_tokens([(b"<x>", 1), (b"<y>", 2), (b"<x>", 3)])
    check(states[3])
    ctx.set_special_tokens([])
    check(states[4])
    ctx.set_byte_fallback(None)
    ctx.set_special_tokens(states[5]["specials"])
    _check_decode_special(ctx, ref, states[5])
    ctx.set_byte_fallback(states[5]["table"])
    check(states[5])
    _check_order_encode(ctx, orc, is_byte, states[5])
    ctx.set_byte_fallback(states[6]["table"])
    check(states[6])
    ctx.close()


def _init(files=None, vocab=None):
    import hutoken_amd
    if files:
        vp, sp, kw = files
        hutoken_amd.initialize(vp, sp, device=0, **kw)
    else:
        hutoken_amd.initialize(vocab[0], vocab[1], prefix="▁", is_byte_encoder=False, device=0)
    return hutoken_amd


@pytest.mark.parametrize("which", ["VL", "char"])
def test_round_trip(tmp_path, vl_files, which):
    import torch
    if which == "VL":
        hu = _init(files=vl_files)
    else:
        ents, special = H.random_char_vocab(5, n_merges=400, drop_chars="e3.")
        hu = _init(vocab=H.write_vocab(tmp_path, "rt", ents, special))
    rng = random.Random(33)
    texts = [H.random_text(rng, max_words=40) for _ in range(3000)]
    plain = hu.batch_encode(texts)
    assert any(-1 in row for row in plain)
    with pytest.raises(ValueError):  # no table yet
        hu.batch_encode_fallback(texts[:3])
    hu.set_byte_fallback()
    ids = hu.batch_encode_fallback(texts)
    assert not any(-1 in row for row in ids)
    assert hu.batch_decode_fallback(ids) == texts
    assert hu.decode_fallback(hu.encode_fallback(texts[7])) == texts[7]
    assert hu.batch_encode(texts) == plain, "batch_encode never looks at the table"
    # with markers
    hu.set_special_tokens({"<|endoftext|>": 32000, "<|im_start|>": 32001})
    marked = ["<|im_start|>" + t + "<|endoftext|>" + t[::-1] for t in texts[:1000]] + ["<|endoftext|>", "", "😂<|im_start|>"]
    mids = hu.batch_encode_fallback(marked, special=True)
    assert all(row.count(32000) + row.count(32001) == t.count("<|") for row, t in zip(mids, marked))
    assert hu.batch_decode_fallback(mids, special=True) == marked
    assert hu.batch_decode_fallback(mids, special=True, skip_special_tokens=True) == \
        hu.batch_decode_fallback([[i for i in row if i not in (32000, 32001)] for row in mids])
    assert hu.decode_fallback(hu.encode_fallback(marked[5], special=True), special=True) == marked[5]
    # device tensors on a stream that is not the default one
    dev = torch.device("cuda", 0)
    data, offs = hu._pack(marked)
    d_bytes, d_offs = torch.from_numpy(data.copy()).to(dev), torch.from_numpy(offs).to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        d_ids, d_oo = hu.encode_fallback_packed_device(d_bytes, d_offs, special=True)
        out, oo = hu.decode_packed_device(d_ids, d_oo, special=True, byte_fallback=True)
        torch.cuda.current_stream(dev).synchronize()
    assert np.array_equal(oo.cpu().numpy(), offs) and out.cpu().numpy().tobytes() == data.tobytes()
    assert d_oo.cpu().tolist() == np.concatenate([[0], np.cumsum([len(r) for r in mids])]).tolist()
    hu.set_special_tokens(None)
    hu.set_byte_fallback(None)


def test_untouched_paths(oracle_mod):
    ctx, orc, is_byte = _shipped(oracle_mod, "VL")
    ctx.set_special_tokens(list(SPECIALS.items()))
    rng = random.Random(8)
    d, o = _pack([("<s>" + H.random_text(rng, max_words=30) + "<|endoftext|>").encode("utf-8") for _ in range(800)])

    def everything():
        ids, oo, st, rc = ctx.encode_packed(d, o)
        known = np.where(ids < 0, ids[ids >= 0][0], ids)  # (the plain decodes refuse -1)
        sp = ctx.token_spans_packed(d, o, ids, oo)
        return [ids, oo, st, *ctx.decode_packed(known, oo), *ctx.encode_special_packed(d, o)[:3],
                *ctx.decode_special_packed(known, oo, 0), *ctx.decode_special_packed(known, oo, 1), sp[0], sp[1]]
    before = everything()
    assert (before[0] == -1).any()
    ctx.set_byte_fallback(ctx.find_byte_tokens()[0])
    ctx.encode_fallback_packed(d, o)
    after = everything()
    assert len(before) == len(after)
    for k, (a, b) in enumerate(zip(before, after)):
        assert np.array_equal(a, b), k
    ctx.close()


def test_refusals(oracle_mod, vg_files):
    from hutoken_amd import _capi
    L = _capi.load()
    ctx, _orc, _b = _shipped(oracle_mod, "VL")
    d, o = _pack([b"abc", "é".encode()])
    ids, offs = np.array([5, 6], np.int32), np.array([0, 2], np.int64)
    with pytest.raises(ValueError, match="no byte-fallback table"):
        ctx.encode_fallback_packed(d, o)
    with pytest.raises(ValueError, match="no byte-fallback table"):
        ctx.decode_fallback_packed(ids, offs)
    assert _dev_encode(ctx, d, o)[5] == E_UNSUPPORTED and _dev_decode(ctx, ids, offs, 0)[5] == E_UNSUPPORTED
    ctx.set_byte_fallback(ctx.find_byte_tokens()[0])
    for flags in (2, 4, 8, -2):  # unknown bits
        assert _dev_encode(ctx, d, o, flags)[5] == E_ARG
        with pytest.raises(TypeError):
            ctx.encode_fallback_packed(d, o, flags)
    for flags in (4, 8, FB_SKIP):  # unknown bits; skip without special
        assert _dev_decode(ctx, ids, offs, flags)[5] == E_ARG
        with pytest.raises(TypeError):
            ctx.decode_fallback_packed(ids, offs, flags)
    ctx.set_pattern(r"[a-z]+")
    assert _dev_encode(ctx, d, o)[5] == E_UNSUPPORTED
    with pytest.raises(ValueError, match="regex"):
        ctx.encode_fallback_packed(d, o)
    ctx.close()
    vp, sp, kw = vg_files
    host = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=-2)
    host.set_byte_fallback(np.arange(1000, 1256))
    out = np.zeros(8, np.int64)
    assert L.hutk_encode_fallback_batch(host.handle, d.ctypes.data, o.ctypes.data, 2, 0, out.ctypes.data, 64, out.ctypes.data, None) == E_DEVICE
    assert L.hutk_decode_fallback_batch(host.handle, ids.ctypes.data, offs.ctypes.data, 1, 0, None, 0, out.ctypes.data, None) == E_DEVICE
    assert L.hutk_encode_fallback_batch_device(host.handle, None, None, 0, 0, 0, None, 0, None, None, None, None) == E_DEVICE
    assert L.hutk_decode_fallback_batch_device(host.handle, None, None, 0, 0, 0, None, 0, None, None, None, None) == E_DEVICE
    host.close()
