"""Special tokens without a GPU: the restatement of tests/specials_ref.py against hand-made cases and Python's `re`, the
new symbols in header, binding and library, the validation of a set on a host-only context, the Python argument checks."""
import os
import random
import re

import numpy as np
import pytest

import helpers as H
import specials_ref as S
from hutoken_amd import _capi

NEW_SYMBOLS = ["hutk_ctx_set_special_tokens", "hutk_ctx_special_token_count", "hutk_special_ids_capacity",
               "hutk_encode_special_batch_device", "hutk_encode_special_batch", "hutk_special_last_matches",
               "hutk_debug_special_tile_bytes"]
EOT = "<|endoftext|>"


def test_split_by_hand():
    assert S.split(b"aaaaa", {b"aa": 7}) == [(0, 2, 7), (2, 4, 7)]
    assert S.split(b"abc", {b"ab": 1, b"bc": 2}) == [(0, 2, 1)]
    assert S.pieces(b"abc", {b"ab": 1, b"bc": 2}) == [b"", 1, b"c"]
    two = {b"<|a|>": 1, b"<|a|><|b": 2}
    assert S.split(b"<|a|><|b|>", two) == [(0, 8, 2)]          # the longer of two at one start
    assert S.split(b"<|a|><|c|>", two) == [(0, 5, 1)]          # the longer fails: the shorter that matches
    assert S.split(b"<|a|><|", two) == [(0, 5, 1)]             # the longer would end behind the document
    assert S.split(b"", {b"a": 1}) == [] and S.pieces(b"", {b"a": 1}) == [b""]
    assert S.pieces(b"xx", {b"x": 3}) == [b"", 3, b"", 3, b""]  # back to back: empty text pieces
    assert S.split(b"bcab", {b"ab": 1, b"bc": 2}) == [(0, 2, 2), (2, 4, 1)]


def test_split_against_re():
    """Leftmost first, then longest, non-overlapping is what `re` finds for the escaped strings joined by |, longest first.
    A three-letter alphabet and lengths 1..5: overlaps and shared prefixes are dense."""
    rng = random.Random(11)
    for _ in range(3000):
        keys = {bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(1, 6))}
        specials = {k: i for i, k in enumerate(sorted(keys))}
        doc = bytes(rng.choice(b"abc") for _ in range(rng.randint(0, 40)))
        pat = re.compile(b"|".join(re.escape(k) for k in sorted(keys, key=len, reverse=True)))
        want = [(m.start(), m.end(), specials[m.group()]) for m in pat.finditer(doc)]
        assert S.split(doc, specials) == want, (doc, specials)


def test_header_binding_and_library_agree_on_the_new_symbols():
    lib = _capi.load()
    header = open(os.path.join(H.ROOT, "include", "hutoken_amd.h")).read()
    declared = set(re.findall(r"\b(hutk_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.hutk_debug_special_tile_bytes() > 0 and lib.hutk_debug_special_tile_bytes() % 16 == 0
    for method in ("set_special_tokens", "special_ids_capacity", "encode_special_packed", "encode_special_device"):
        assert hasattr(_capi.Context, method), method


def _host_ctx(files):
    vp, sp, kw = files
    return _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=-2)


def test_a_host_only_context_validates_the_set(vg_files):
    ctx = _host_ctx(vg_files)
    assert ctx.special_token_count == 0
    ctx.set_special_tokens([(EOT.encode(), 50256), (b"<|im_start|>", 50257)])
    assert ctx.special_token_count == 2
    bad = {
        "empty": [(b"", 1)],
        "equal": [(b"<a>", 1), (b"<b>", 2), (b"<a>", 3)],
        "0x00": [(b"a\0b", 1)],
        "1024": [(b"<%d>" % i, i) for i in range(1025)],
        "255": [(b"x" * 256, 1)],
        "negative": [(b"<a>", -1)],
    }
    for word, pairs in bad.items():
        with pytest.raises(ValueError, match=word):
            ctx.set_special_tokens(pairs)
        assert ctx.special_token_count == 2, word  # a refused set leaves the one in force
    # the largest set there is: 1024 strings of 255 bytes, ids that are no vocabulary lines
    big = [(b"<" + b"%04d" % i + b"y" * 250, 2**31 - 1 - i) for i in range(1024)]
    assert all(len(k) == 255 for k, _ in big)
    ctx.set_special_tokens(big)
    assert ctx.special_token_count == 1024
    ctx.set_special_tokens([])
    assert ctx.special_token_count == 0
    # no device: the encode fails loudly, after the arguments were looked at
    ctx.set_special_tokens([(EOT.encode(), 50256)])
    with pytest.raises(RuntimeError, match="host-only"):
        ctx.encode_special_packed(np.frombuffer(b"abc", dtype=np.uint8), np.array([0, 3], dtype=np.int64))
    ctx.close()


def test_capacity_bound(vg_files, vl_files):
    """n_bytes x max(U, P + 1) + n_docs x P + 1 (the header's proof), never below the plain capacity."""
    for files in (vg_files, vl_files):
        ctx = _host_ctx(files)
        pad = ctx.ids_capacity(0, 1) - 1
        units = ctx.ids_capacity(1, 0) - 1
        assert (pad > 0) == (files[2]["prefix"] is not None)
        for n_bytes, n_docs in ((0, 0), (0, 5), (1, 1), (1000, 3), (10**9, 10**6)):
            cap = ctx.special_ids_capacity(n_bytes, n_docs)
            assert cap == n_bytes * max(units, pad + 1) + n_docs * pad + 1
            assert cap >= ctx.ids_capacity(n_bytes, n_docs)
        ctx.close()


def test_python_argument_checks_come_first():
    """TypeError / ValueError for a bad mapping whatever the state of the context: nothing reaches the library."""
    import hutoken_amd
    for bad in (5, "x", [("a", 1)], {b"a": 1}, {"a": "1"}, {"a": 1.0}, {"a": True}, {1: 1}):
        with pytest.raises(TypeError):
            hutoken_amd.set_special_tokens(bad)
    many = {"<%d>" % i: i for i in range(1025)}
    for bad in ({"": 1}, {"a\0b": 1}, {"x" * 256: 1}, {"é" * 128: 1}, {"a": -1}, {"a": 2**31}, many):
        with pytest.raises(ValueError):
            hutoken_amd.set_special_tokens(bad)
    with pytest.raises(TypeError):
        hutoken_amd.encode_special(5)
    with pytest.raises(ValueError):
        hutoken_amd.encode_special("a\0b")
    with pytest.raises(TypeError):
        hutoken_amd.batch_encode_special("not a list")


def test_the_reference_cuts_a_marker_into_eight_ids(oracle_mod, vg_files):
    """What the feature is for: the plain encode gives eight ids for the marker, the contract's encoding one."""
    vp, sp, kw = vg_files
    orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    assert orc.encode(EOT) == [27, 91, 405, 463, 7538, 11344, 91, 29]
    d, o = oracle_mod.pack(["a" + EOT + "b", EOT, "", "no marker here"])
    ids, oo, st, matches = S.encode(orc, d, o, {EOT.encode(): 50256})
    assert matches == 2 and not st.any()
    assert ids[int(oo[0]):int(oo[1])].tolist() == orc.encode("a") + [50256] + orc.encode("b")
    assert ids[int(oo[1]):int(oo[2])].tolist() == [50256] and oo[2] == oo[3]
    assert ids[int(oo[3]):].tolist() == orc.encode("no marker here")
