"""The vocabularies and documents of tests/exc_cases.py are what they claim to be, so that no test of
tests/test_gpu_exc_kinds.py passes vacuously: each kind's tables are of the tabled kind, every limit is hit in every
position, the words really merge, the batches have the shapes that reach the three tails, and the oracle cuts no
document.  Host-only contexts (device = -2) and the oracle.  No GPU."""
import statistics

import numpy as np
import pytest

import exc_cases as X

KIND_TAGS = list(X.KINDS)
SYM16_LIMIT = 65520


@pytest.fixture(scope="module")
def made(tmp_path_factory, oracle_mod):
    """tag -> (Kind, oracle, the oracle's (ids, offsets, status) of the full batch), each made once."""
    tmp = tmp_path_factory.mktemp("exc")
    cache = {}

    def get(tag):
        if tag not in cache:
            k = X.kind(tag, tmp)
            orc = X.oracle(k, oracle_mod)
            data, offs = oracle_mod.pack(X.full_docs(k))
            cache[tag] = (k, orc, orc.encode_packed(data, offs, num_threads=4))
        return cache[tag]
    return get


def test_the_list_rule_restated():
    """list_of on hand-made kinds: the limits of exc_list_of, and which kinds have which lists."""
    K = lambda **kw: X.Kind(**{**dict.fromkeys(X.Kind._fields), **kw})
    fast = K(is_byte=True, sym32=False, rank_is_sym=True, multi=False)
    assert [X.list_of(fast, n) for n in (64, 128, 129, 256, 257, 512, 513, 1024, 1025, 3000)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    quad = K(is_byte=True, sym32=True, rank_is_sym=True, multi=False)
    assert [X.list_of(quad, n) for n in (64, 128, 129, 256, 257, 1024)] == [0, 0, 1, 1, 4, 4]
    for other in (K(is_byte=False, sym32=True, rank_is_sym=True, multi=False), K(is_byte=True, sym32=False, rank_is_sym=False, multi=False),
                  K(is_byte=True, sym32=False, rank_is_sym=True, multi=True), K(is_byte=True, sym32=True, rank_is_sym=False, multi=False)):
        assert {X.list_of(other, n) for n in (64, 128, 256, 512, 1024, 2046)} == {4}
    char_fast = K(is_byte=False, sym32=False, rank_is_sym=True, multi=False)
    assert X.list_of(char_fast, 100) == 0 and X.list_of(char_fast, 600) == 3
    assert X.wave_lds_route(fast, 2046, small=False) == "lds" and X.wave_lds_route(fast, 2046, small=True) == "hbm"
    assert X.wave_lds_route(fast, 2047, small=False) == "hbm" and X.wave_lds_route(quad, 1025, small=False) == "hbm"
    assert X.wave_lds_route(quad, 1024, small=True) == "lds"


def test_the_words_of_a_document_restated(oracle_mod):
    """gpu_words and units on hand-made documents: the reference's starts, a seam's cut, the prefix and an item of five."""
    sw = oracle_mod.split_words
    assert X.gpu_words(b"ab cd", None, sw) == [(0, 2), (2, 5)]
    doc = "ab漢字".encode("utf-8")
    assert X.gpu_words(doc, None, sw) == [(0, 2), (2, 8)]
    none_join = [0] * 256  # no merge joins anything to a three-byte character: every one of them starts a word
    assert X.gpu_words(doc, none_join, sw) == [(0, 2), (2, 5), (5, 8)]
    all_join = [0xFFFFFFFF] * 256
    assert X.gpu_words(doc, all_join, sw) == [(0, 2), (2, 8)]
    K = lambda **kw: X.Kind(**{**dict.fromkeys(X.Kind._fields), **kw})
    ch = K(is_byte=False, prefix="▁▁", n_prefix=2, scale={ord("q"): 5}, multi=True)
    d = "aéq b".encode("utf-8")
    assert X.units(ch, d, 0, 4) == 2 + 2 + 5 and X.units(ch, d, 4, 6) == 2
    assert X.units(ch, b" ab", 0, 3) == 3  # (the document begins with a space: the prefix is a word of its own)
    by = K(is_byte=True, prefix=None, n_prefix=0, scale={}, multi=False)
    assert X.units(by, d, 0, 4) == 4


def test_the_room_for_prefixes_restated(oracle_mod):
    """list_counts on hand-made batches of a character kind with items of several units: a tile gives four document-first
    words a place for their prefix units; the others are exception words, and d_exc's."""
    K = lambda **kw: X.Kind(**{**dict.fromkeys(X.Kind._fields), **kw})
    ch = K(is_byte=False, prefix="▁", n_prefix=1, scale={ord("q"): 5}, multi=True, sym32=False, rank_is_sym=True)
    sw = oracle_mod.split_words
    short, long40 = b"abc def", b"e" * 40 + b" x"
    assert X.list_counts(ch, [short] * 4, None, sw)[:2] == ([0, 0, 0, 0, 0], 0)
    assert X.list_counts(ch, [short] * 6, None, sw)[:2] == ([0, 0, 0, 0, 2], 0)
    assert X.list_counts(ch, [long40] * 6, None, sw)[:2] == ([0, 0, 0, 0, 6], 0)  # (more than 32 units: d_exc's anyway)
    assert X.list_counts(ch, [b" " + short] * 6 + [b"aqc"] * 6, None, sw)[:2] == ([0, 0, 0, 0, 6], 0)  # (neither asks for a place)
    assert X.list_counts(ch, [short] * 5 + [long40], None, sw)[1] > 0  # which of the six goes without is not defined
    far = [short] * 4 + [b"e" * 100 + b" " + b"t" * 900] + [short] * 4  # the second four are in the next tile
    assert X.list_counts(ch, far, None, sw)[:2] == ([0, 0, 0, 0, 2], 0)
    by = K(is_byte=True, prefix=None, n_prefix=0, scale={ord("q"): 5}, multi=True, sym32=False, rank_is_sym=True)
    assert X.list_counts(by, [short] * 6, None, sw)[:2] == ([0, 0, 0, 0, 0], 0)


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_kind_is_as_tabled(made, tag):
    k = made(tag)[0]
    ctx = X.host_context(k)
    st = ctx.table_stats()
    assert (st["n_sym"] >= SYM16_LIMIT) == k.sym32, st
    assert bool(st["rank_is_sym"]) == k.rank_is_sym, st
    assert ctx.uses_merges == k.merges
    if k.multi:
        assert ctx.ids_capacity(100, 0) >= 500  # five or six units per item: more ids than bytes are possible
    else:
        assert ctx.ids_capacity(100, 0) < 200
    assert len(k.pieces["1"]) >= 10 and (k.is_byte or (len(k.pieces["12"]) >= 20 and len(k.pieces["3"]) >= 5))
    ctx.close()


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_every_limit_is_hit_in_every_position(made, oracle_mod, tag):
    k = made(tag)[0]
    sw = oracle_mod.split_words
    seen, wide, cjk, items = set(), set(), set(), set()
    for doc, form, u, _cls in X.limit_docs(k):
        words = X.gpu_words(doc, k.seams, sw)
        at = [i for i, (a, b) in enumerate(words) if X.units(k, doc, a, b) == u]
        assert at, (tag, form, u)
        i = at[0]
        a, b = words[i]
        # the position is the claimed one
        if form in ("alone", "short-behind", "long-behind"):
            assert a == 0 and X.gets_prefix(k, doc, a) == bool(k.prefix)
        elif form == "space-first":
            assert doc[:1] == b" " and a <= 1 and not X.gets_prefix(k, doc, a)
        else:
            assert a > 1 and not X.gets_prefix(k, doc, a)
        if form == "alone":
            assert i == len(words) - 1 and b == len(doc)
        if form == "short-behind":
            assert len(doc) - b <= 8 and b < len(doc)
        if form == "long-behind":
            assert X.units(k, doc, *words[-1]) >= min(u, 31) - 1 and len(words) > i + 1
        seen.add((form, u))
        w = doc[a:b]
        if b - a > X.own_units(k, w):
            wide.add(u)
        if all(c >= 0x80 for c in w.lstrip(b" ")):
            cjk.add(u)
        n_items = sum(c == ord("q") for c in w) if k.multi else 0
        if n_items:
            assert sum((c & 0xC0) != 0x80 for c in w) < u - 3  # the items (bytes, characters) stay below the limit the units are on
            items.add((u, n_items))
    assert seen == {(f, u) for f in X.FORMS for u in X.LIMITS}
    if not k.is_byte:  # bytes != units: every limit with two-byte letters in the word, and as a run of three-byte characters
        assert wide == set(X.LIMITS) and cjk == set(X.LIMITS), (sorted(wide), sorted(cjk))
    if k.multi:
        assert {(u, n) for u in X.LIMITS if u >= 127 for n in (1, 2, 13)} <= items
        assert {(u, n) for u in X.LIMITS for n in (1, 2)} <= items


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_positions_across_tiles_and_items(made, oracle_mod, tag):
    """In the full batch long words end 0, 1, 2 and 3 tiles beyond the tile they start in, the batch ends with a long word,
    and (kinds with q -> "Alpha") an item sits at bytes 0, 63, 64 and last of a 64-byte step of the expansion."""
    k = made(tag)[0]
    docs = X.full_docs(k)
    assert X.tiles_of(docs) > 4 * X.SMALL_TILES
    sw = oracle_mod.split_words
    beyond, base, item_at = set(), 0, set()
    for doc in docs:
        for a, b in X.gpu_words(doc, k.seams, sw):
            if b - a > X.LANE_MAX_BYTES:
                beyond.add((base + b - 1) // X.TILE - (base + a) // X.TILE)
                if k.multi:
                    w = doc[a:b]
                    item_at |= {("first" if i == 0 else "last" if i == len(w) - 1 else i % 64)
                                for i, c in enumerate(w) if c == ord("q")}
        base += len(doc)
    assert {0, 1, 2, 3} <= beyond
    a, b = X.gpu_words(docs[-1], k.seams, sw)[-1]
    assert a == 0 and b == len(docs[-1]) and b - a > X.LANE_MAX_BYTES
    if k.multi:
        assert {"first", "last", 0, 63} <= item_at
        assert any(d == b"q" * 5000 for d in docs) and any(d == b"aqb " * 2000 for d in docs)
    if ord("\t") in k.scale:
        assert any(d == b"\t" * 5000 for d in docs) and any(d == b"a\tb " * 2000 for d in docs)


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_the_words_really_merge(made, tag):
    """The oracle's ids per unit over the long words (65 units and more, alone in their document): a median of at most
    0.8, and at most 5 % of all ids are -1.  (Random letters give about 1.0 under these vocabularies; the glued keys gave
    medians of 0.32 .. 0.68 and, in C16xm, 2.9 % of -1 -- the Llama file's "<0x09>" units that have no rule.)"""
    k, _orc, (ids, oo, _st) = made(tag)
    ratios = [(oo[i + 1] - oo[i]) / u for i, (_d, form, u, _c) in enumerate(X.limit_docs(k)) if form == "alone" and u >= 65]
    assert len(ratios) >= len([u for u in X.LIMITS if u >= 65])
    assert statistics.median(ratios) <= 0.8, (tag, statistics.median(ratios))
    assert float((ids < 0).mean()) <= 0.05, (tag, float((ids < 0).mean()))


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_batch_shapes_are_as_claimed(made, oracle_mod, tag):
    k = made(tag)[0]
    docs = X.full_docs(k)
    sw = oracle_mod.split_words
    counts, unknown, _listed = X.list_counts(k, docs, k.seams, sw)
    used = {X.list_of(k, n) for n in (100, 200, 400, 800, 1500)}
    assert all(counts[li] >= 10 for li in set(used)), counts
    assert all(counts[li] == 0 for li in range(5) if li not in used), counts
    assert unknown == 0, unknown  # (every word's list can be told: no tile mixes short and long first words past its four places)
    batches, left_out = X.small_batches(docs)
    assert not left_out and sum(len(b) for b in batches) == len(docs) and len(batches) >= 10
    every_list, hbm_word = 0, 0
    for b in batches:
        assert 5 <= X.tiles_of(b) <= X.SMALL_TILES and len(b) <= X.SMALL_DOCS
        c, u, listed = X.list_counts(k, b, k.seams, sw)
        assert u == 0
        every_list += all(c[li] > 0 for li in set(used))
        hbm_word += any(li == 4 and 1025 <= X.units(k, b[d], x, y) <= 2046 for d, x, y, li in listed)
    assert every_list >= 1 and hbm_word >= 1
    if tag in X.ONE_LAUNCH_KINDS:
        ones = X.one_launch_batches(k)
        assert len(ones) >= 3 * len([u for u in X.LIMITS if u <= 1025])
        assert all(1 <= X.tiles_of(b) <= X.ONE_TILES for b in ones) and any(len(b) == 2 for b in ones)
        assert max(sum(len(d) for d in b) for b in ones) > 3 * X.TILE
    else:
        assert k.multi


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_every_status_is_zero(made, oracle_mod, tag):
    k, orc, (_ids, oo, st) = made(tag)
    assert (st == 0).all() and (np.diff(oo) > 0).all()
    if tag in X.GIANT_KINDS:
        docs = X.giant_docs(k)
        sw = oracle_mod.split_words
        got = sorted(max(X.units(k, d, a, b) for a, b in X.gpu_words(d, k.seams, sw)) for d in docs)
        assert got == list(X.GIANT)
        data, offs = oracle_mod.pack(docs)
        _i, _o, st = orc.encode_packed(data, offs, num_threads=2)
        assert (st == 0).all()


def test_the_diagnostic_needs_a_device(made):
    """hutk_debug_exc_counts reports a device-form encode: a host-only context has none to report."""
    ctx = X.host_context(made("B16")[0])
    with pytest.raises(Exception, match="host-only"):
        ctx.exc_counts()
    ctx.close()
