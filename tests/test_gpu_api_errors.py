"""What the host-buffer entry points of the C API answer to bad arguments: the return code and the text of
hutk_last_error(), for hutk_encode_batch (the hand-written splitter and a regex pattern), hutk_decode_batch,
hutk_token_spans and hutk_trainer_add, on two documents of a few bytes.

Every expected text is the one the entry point's source spells out.  Every case is one call that ends in an argument or a
capacity error: the offsets are refused on the host before anything is copied, a capacity that is one too small and an id
outside the vocabulary are what the decode kernels themselves report (tests/test_gpu_decode_edges.py).  hutk_trainer_add
takes offsets that begin above 0 (they address a larger buffer): that case pins HUTK_OK.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

OK, E_VALUE, E_ARG, E_CAPACITY = 0, 2, 4, 7
DOCS = [b"ab", b"cd e"]
DATA = np.frombuffer(b"".join(DOCS), dtype=np.uint8).copy()
OFFS = [0, 2, 6]
FIRST_ONE, DECREASING = [1, 2, 6], [0, 4, 2]


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """-> (library, context, the documents' ids, their id offsets)"""
    from hutoken_amd import _capi
    ents, special = H.random_byte_vocab(3, n_merges=300)
    vp, sp = H.write_vocab(tmp_path_factory.mktemp("api_errors"), "v", ents, special)
    ctx = _capi.Context(vp, sp, None, True, device=0)
    ids, oo, _st, rc = ctx.encode_packed(DATA, OFFS)
    assert rc == OK and oo[0] == 0 and oo[2] == len(ids) > 0
    text, _too, _st = ctx.decode_packed(ids, oo)
    assert text.tobytes() == DATA.tobytes()
    yield _capi.load(), ctx, np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(oo, dtype=np.int64)
    ctx.close()


def i64(v):
    return np.asarray(v, dtype=np.int64)


def expect(rc, code, text):
    from hutoken_amd import _capi
    print("rc %d, last error %r" % (rc, _capi.last_error()))
    assert rc == code
    if code != OK:
        assert _capi.last_error() == text


ENCODE_CASES = {
    "first_offset_one": (FIRST_ONE, True, 0, E_ARG, "offsets[0] must be 0"),
    "decreasing": (DECREASING, True, 0, E_ARG, "offsets must not decrease"),
    "null_bytes": (OFFS, False, 0, E_ARG, "bad argument"),
    "ids_cap_one_short": (OFFS, True, -1, E_CAPACITY, "ids_cap is below hutk_ids_capacity()"),
}


@pytest.mark.parametrize("pattern", [None, "[a-z]+"], ids=["plain", "pattern"])
@pytest.mark.parametrize("case", sorted(ENCODE_CASES))
def test_encode_batch(env, case, pattern):
    L, ctx, _ids, _oo = env
    offsets, with_bytes, cap_delta, code, text = ENCODE_CASES[case]
    offs = i64(offsets)
    need = ctx.ids_capacity(len(DATA), 2) - 1  # (what the entry point asks for)
    ids = np.zeros(need + 1, dtype=np.int32)
    oo, st = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int32)
    ctx.set_pattern(pattern)
    try:
        rc = L.hutk_encode_batch(ctx.handle, DATA.ctypes.data if with_bytes else None, offs.ctypes.data, 2, ids.ctypes.data,
                                 need + cap_delta, oo.ctypes.data, st.ctypes.data)
        expect(rc, code, text)
    finally:
        ctx.set_pattern(None)


DECODE_CASES = {
    # name: (id offsets or None for the documents' own, ids: "own" / "null" / "bad", bytes_cap - total, code, text)
    "first_offset_one": (FIRST_ONE, "own", 0, E_ARG, "id_offsets[0] must be 0"),
    "decreasing": (DECREASING, "own", 0, E_ARG, "id_offsets must not decrease"),
    "null_ids": (None, "null", 0, E_ARG, "bad argument"),
    "bytes_cap_one_short": (None, "own", -1, E_CAPACITY, "bytes_cap too small"),
    "id_out_of_range": (None, "bad", 0, E_VALUE, "Element must be non-negative and less than vocab size."),
}


@pytest.mark.parametrize("case", sorted(DECODE_CASES))
def test_decode_batch(env, case):
    L, ctx, ids0, oo0 = env
    offsets, which, cap_delta, code, text = DECODE_CASES[case]
    ids = ids0.copy()
    if which == "bad":
        ids[-1] = L.hutk_vocab_size(ctx.handle) + 7
    id_offs = oo0 if offsets is None else i64(offsets)
    if offsets is not None:  # (refused before the ids are looked at; they only have to be there)
        ids = np.zeros(8, dtype=np.int32)
    out = np.zeros(len(DATA) + 16, dtype=np.uint8)
    oo, st = np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int32)
    rc = L.hutk_decode_batch(ctx.handle, None if which == "null" else ids.ctypes.data, id_offs.ctypes.data, 2,
                             out.ctypes.data, len(DATA) + cap_delta, oo.ctypes.data, st.ctypes.data)
    expect(rc, code, text)


SPANS_CASES = {
    # name: (document offsets, id offsets or None for the documents' own, with bytes, code, text)
    "first_id_offset_one": (OFFS, FIRST_ONE, True, E_ARG, "offsets[0] must not be negative, id_offsets[0] must be 0"),
    "first_offset_negative": ([-1, 2, 6], None, True, E_ARG, "offsets[0] must not be negative, id_offsets[0] must be 0"),
    "decreasing": (DECREASING, None, True, E_ARG, "offsets must not decrease"),
    "decreasing_id_offsets": (OFFS, DECREASING, True, E_ARG, "offsets must not decrease"),
    "null_bytes": (OFFS, None, False, E_ARG, "hutk_token_spans: a buffer is NULL"),
}


@pytest.mark.parametrize("case", sorted(SPANS_CASES))
def test_token_spans(env, case):
    from hutoken_amd import _capi
    L, ctx, ids0, oo0 = env
    offsets, id_offsets, with_bytes, code, text = SPANS_CASES[case]
    offs = i64(offsets)
    id_offs = oo0 if id_offsets is None else i64(id_offsets)
    ids = np.zeros(max(len(ids0), 8), dtype=np.int32)
    ids[:len(ids0)] = ids0
    spans = np.zeros(2 * len(ids), dtype=np.int32)
    st = np.zeros(2, dtype=np.int32)
    rc = L.hutk_token_spans(ctx.handle, DATA.ctypes.data if with_bytes else None, offs.ctypes.data, 2, ids.ctypes.data,
                            id_offs.ctypes.data, _capi.SPANS_BYTES, 4, spans.ctypes.data, st.ctypes.data)
    expect(rc, code, text)


TRAINER_CASES = {
    "first_offset_one": (FIRST_ONE, True, OK, None),
    "first_offset_negative": ([-1, 2, 6], True, E_ARG, "hutk_trainer_add: offsets must not decrease"),
    "decreasing": (DECREASING, True, E_ARG, "hutk_trainer_add: offsets must not decrease"),
    "null_bytes": (OFFS, False, E_ARG, "hutk_trainer_add: bytes is NULL"),
}


@pytest.mark.parametrize("case", sorted(TRAINER_CASES))
def test_trainer_add(env, case):
    L = env[0]
    offsets, with_bytes, code, text = TRAINER_CASES[case]
    offs = i64(offsets)
    data = np.zeros(64, dtype=np.uint8)  # (the documents in front of a buffer that is larger than they are)
    data[:len(DATA)] = DATA
    h = C.c_void_p()
    assert L.hutk_trainer_create(C.byref(h), 0) == OK
    try:
        rc = L.hutk_trainer_add(h, data.ctypes.data if with_bytes else None, offs.ctypes.data, 2)
        expect(rc, code, text)
    finally:
        L.hutk_trainer_destroy(h)
