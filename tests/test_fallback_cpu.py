"""Byte fallback without a GPU: the plain restatement (tests/fallback_ref.py) on the shipped Llama-shaped vocabulary --
the plain ids hold -1, the restated encode holds none, stays within the capacity and decodes back to the text -- and the
host side of the C API and of the Python layer.  The GPU is compared with the restatement in tests/test_gpu_fallback.py."""
import ctypes as C
import random

import numpy as np
import pytest

import fallback_ref as F
import helpers as H
import spans_ref as S

E_VALUE = 2


def _pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in docs], out=offs[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


def _host_ctx(files):
    from hutoken_amd import _capi
    vp, sp, kw = files
    return _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=-2)


def _batch(which):
    from hutoken_amd import synth
    if which == "random_text":
        rng = random.Random(5)
        return _pack([H.random_text(rng, max_words=40).encode("utf-8") for _ in range(3000)])
    return synth.corpus(which, {"C2": 300, "C3": 1500}[which])


@pytest.mark.parametrize("which", ["C2", "C3", "random_text"])
def test_restatement_on_the_llama_shaped_vocabulary(oracle_mod, vl_files, which):
    vp, sp, kw = vl_files
    orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    ctx = _host_ctx(vl_files)
    table, found = ctx.find_byte_tokens()
    assert found == 256
    d, o = _batch(which)
    ids, oo, st = orc.encode_packed(d, o, 4)
    assert (ids == -1).any(), "the plain encode of this batch holds ids of -1"
    assert not st.any()
    tt = S.TokenText(orc)
    got, goo, mism = F.encode(tt, d, o, ids, oo, kw["is_byte_encoder"], table)
    assert not mism.any()
    assert (got >= 0).all(), "the restated fallback encode holds no -1"
    assert len(got) == goo[-1] and len(got) >= len(ids)  # (an unknown item of one byte gives one id)
    assert len(got) <= ctx.ids_capacity(int(o[-1]), len(o) - 1) - 1
    known = ids != -1
    assert np.array_equal(got[~np.isin(got, table)], ids[known & ~np.isin(ids, table)])  # known ids, in order
    out, out_oo, dst = F.decode_packed(F.from_token_text(tt, 1 << 30), got, goo, table)
    assert not dst.any()
    assert np.array_equal(out_oo, o) and out.tobytes() == np.asarray(d).tobytes()
    ctx.close()


def test_expansion_by_hand():
    table = [1000 + b for b in range(256)]
    doc = "aé😂".encode()
    ids, spans = [7, -1, -1], [(0, 1), (1, 3), (3, 7)]
    assert F.expand_doc(doc, ids, spans, False, table) == [7, 1000 + 0xC3, 1000 + 0xA9, 1000 + 0xF0, 1000 + 0x9F, 1000 + 0x98, 1000 + 0x82]
    assert F.expand_doc(doc, ids, spans, True, table) == ids  # a document whose spans do not verify keeps its ids
    tokens = lambda i, first: ((b"" if first else b" ") + b"a", 0) if i == 7 else (b"", 3)
    assert F.decode_doc(tokens, [1000 + 0xC3, 1000 + 0xA9, 7], table) == ("é a".encode(), 0)  # not stripped behind a fallback id
    assert F.decode_doc(tokens, [7, 1000 + 0x41], table) == (b"aA", 0)
    assert F.decode_doc(tokens, [7, 5, 1000 + 0x41], table) == (b"aA", 3)  # a bad id contributes nothing
    sp = [(b"<s>", 9)]
    assert F.decode_doc(tokens, [9, 7, 1000 + 0x41, 9, 7], table, sp) == (b"<s>aA<s>a", 0)
    assert F.decode_doc(tokens, [9, 7, 1000 + 0x41, 9, 7], table, sp, skip=True) == (b"aA a", 0)
    assert F.decode_doc(tokens, [9, 1000 + 0x41, 7], table, sp, skip=True) == (b"A a", 0)


def test_find_byte_tokens(oracle_mod, vl_files, vg_files):
    vp, sp, kw = vl_files
    orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    ctx = _host_ctx(vl_files)
    table, found = ctx.find_byte_tokens()
    assert found == 256 and table.dtype == np.int32 and len(set(table.tolist())) == 256
    for b in range(256):
        assert orc.lookup(b"<0x%02X>" % b) == table[b], b
    ctx.close()
    ctx = _host_ctx(vg_files)
    table, found = ctx.find_byte_tokens()
    assert found == 0 and (table == -1).all()
    ctx.close()


def test_set_byte_fallback_on_a_host_only_context(vl_files):
    from hutoken_amd import _capi
    lib = _capi.load()
    ctx = _host_ctx(vl_files)
    assert ctx.byte_fallback is None  # a new context starts without a table
    table, _ = ctx.find_byte_tokens()
    ctx.set_byte_fallback(table)
    assert np.array_equal(ctx.byte_fallback, table)
    other = np.arange(100000, 100256, dtype=np.int32)  # ids need not be vocabulary lines
    ctx.set_byte_fallback(other)
    assert np.array_equal(ctx.byte_fallback, other)
    for bad in (np.where(np.arange(256) == 17, -1, other), np.where(np.arange(256) == 200, other[3], other)):
        bad = np.ascontiguousarray(bad, dtype=np.int32)
        assert lib.hutk_ctx_set_byte_fallback(ctx.handle, bad.ctypes.data) == E_VALUE
        assert np.array_equal(ctx.byte_fallback, other), "a refused table leaves the one in force"
        with pytest.raises(ValueError):
            ctx.set_byte_fallback(bad)
    assert lib.hutk_ctx_byte_fallback(ctx.handle, None) == 1
    ctx.set_byte_fallback(None)
    assert ctx.byte_fallback is None and lib.hutk_ctx_byte_fallback(ctx.handle, None) == 0
    out = (C.c_int32 * 256)()
    assert lib.hutk_ctx_find_byte_tokens(None, out) == 0 and lib.hutk_ctx_byte_fallback(None, None) == 0
    ctx.close()


def test_auto_needs_all_256_lines(vg_files, vl_files, monkeypatch):
    import hutoken_amd
    monkeypatch.setattr(hutoken_amd, "_ctx", _host_ctx(vg_files))
    with pytest.raises(ValueError, match="<0x00>"):
        hutoken_amd.set_byte_fallback("auto")
    monkeypatch.setattr(hutoken_amd, "_ctx", _host_ctx(vl_files))
    hutoken_amd.set_byte_fallback()
    want, _ = hutoken_amd._ctx.find_byte_tokens()
    assert np.array_equal(hutoken_amd._ctx.byte_fallback, want)
    hutoken_amd.set_byte_fallback(None)
    assert hutoken_amd._ctx.byte_fallback is None


def test_python_argument_checks_come_first():
    """TypeError / ValueError for a bad argument whatever the state of the context: nothing reaches the library."""
    import hutoken_amd
    ok = list(range(256))
    for bad in (5, "x", b"auto", 1.5, ok[:-1] + [1.0], ok[:-1] + [True], ok[:-1] + ["7"]):
        with pytest.raises(TypeError):
            hutoken_amd.set_byte_fallback(bad)
    for bad in (ok[:-1], ok + [256], ok[:-1] + [-1], ok[:-1] + [2**31], ok[:-1] + [3], []):
        with pytest.raises(ValueError):
            hutoken_amd.set_byte_fallback(bad)
    with pytest.raises(TypeError):
        hutoken_amd.encode_fallback(b"bytes")
    with pytest.raises(ValueError):
        hutoken_amd.encode_fallback("a\0b")
    with pytest.raises(TypeError):
        hutoken_amd.batch_encode_fallback("not a list")
    with pytest.raises(TypeError):
        hutoken_amd.batch_encode_fallback(["a"], special="yes")
    for f in (hutoken_amd.decode_fallback, hutoken_amd.batch_decode_fallback):
        with pytest.raises(ValueError, match="special=True"):
            f([[1]], skip_special_tokens=True)
        with pytest.raises(TypeError):
            f([[1]], special="yes")
        with pytest.raises(TypeError):
            f([[1]], special=True, skip_special_tokens="no")
    with pytest.raises(TypeError):
        hutoken_amd.decode_packed_device(None, None, byte_fallback="yes")
    with pytest.raises(ValueError):
        hutoken_amd.decode_packed_device(None, None, skip_special_tokens=True, byte_fallback=True)
    assert {"set_byte_fallback", "encode_fallback", "batch_encode_fallback", "encode_fallback_packed_device",
            "decode_fallback", "batch_decode_fallback"} <= set(hutoken_amd.__all__)
