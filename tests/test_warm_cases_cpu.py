"""The batches of tests/warm_cases.py are what they claim to be, so that no test of tests/test_gpu_warm_context.py passes
vacuously: every planted word has the stated length and id count, is one word for the splitter where it stands, needs
the merge loop where the case wants a cached word, and lies where it is said to lie relative to a tile edge; the
overflow batch gives every sub-list more than twice its capacity in candidates.  The oracle only.  No GPU."""
import os
import re

import numpy as np
import pytest

import helpers as H
import specials_ref as SR
import warm_cases as WC


@pytest.fixture(scope="module")
def orc(oracle_mod, vg_files):
    vp, sp, kw = vg_files
    assert kw["is_byte_encoder"] and kw["prefix"] is None
    o = oracle_mod.Oracle(vp, sp, None, True)
    yield o
    o.close()


def _header(name):
    with open(os.path.join(H.ROOT, "hutoken_amd", "csrc", name), encoding="utf-8") as f:
        return f.read()


def _const(text, name):
    m = re.search(r"\b%s = ([0-9a-fx<u ]+?)[,;]" % name, text)
    assert m, name
    return int(eval(m.group(1).replace("u", "")))  # ("1u << 20", "256", "30")


def test_the_constants_are_the_headers():
    wc, dev, ker = _header("hutk_wcache.h"), _header("hutk_device.h"), _header("hutk_kernels.hip")
    assert WC.KEY_BYTES == _const(wc, "KEY_BYTES") and WC.MIN_BYTES == _const(wc, "MIN_BYTES") and WC.MAX_IDS == _const(wc, "MAX_IDS")
    assert WC.LIST_CAP == _const(wc, "LIST_CAP") and WC.LIST_SHARDS == _const(wc, "LIST_SHARDS")
    assert "SHARD_CAP = LIST_CAP / LIST_SHARDS" in wc and WC.SHARD_CAP == WC.LIST_CAP // WC.LIST_SHARDS == 4096
    assert WC.TILE == _const(dev, "TILE_BYTES") and WC.LANE_MAX_BYTES == _const(dev, "LANE_MAX_BYTES")
    assert WC.TILE_WAVES == _const(ker, "TILE_WAVES")
    # the rules the restatements rest on, as the kernel writes them
    assert "blockIdx.x & (wc::LIST_SHARDS - 1u)" in ker
    assert "(int64_t)(blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3)" in ker
    assert "((a.n_tiles + WV - 1) / WV + 7) / 8 * 8" in ker
    assert "r0 += 64" in ker and WC.ROUND == 64


def test_the_block_order_restated():
    """shard_of_group against a loop over the blocks of a small grid and of the overflow batch's"""
    for n_bytes in (WC.LARGE, 100 * WC.GROUP + 7, WC.overflow_size() + 3):
        n_tiles = -(-n_bytes // WC.TILE)
        grid = (-(-n_tiles // WC.TILE_WAVES) + 7) // 8 * 8
        blocks = np.arange(grid)
        groups = (blocks & 7) * (grid >> 3) + (blocks >> 3)
        assert sorted(groups.tolist()) == list(range(grid))
        assert np.array_equal(WC.shard_of_group(groups, n_bytes), blocks & (WC.LIST_SHARDS - 1))


def test_overflow_batch(orc, oracle_mod):
    data, offs, starts = WC.overflow_batch()
    n = len(data)
    assert n == int(offs[-1]) and WC.overflow_size() <= n < WC.overflow_size() + WC.OVER_MAX_WORD
    assert 20e6 < n < 25e6
    # every word: a space and 6 .. 8 rare letters, 7 .. 9 bytes
    lens = np.diff(np.concatenate((starts, [n])))
    assert lens.min() == 7 and lens.max() == WC.OVER_MAX_WORD == 9
    assert (data[starts] == 0x20).all()
    space = data == 0x20
    assert int(space.sum()) == len(starts), "a space that begins no word"
    assert np.isin(data[~space], np.frombuffer(WC.RARE, dtype=np.uint8)).all()
    assert 2.2 * WC.LIST_CAP < len(starts) < 2.6 * WC.LIST_CAP
    # pairwise distinct: the words as fixed-width records
    rec = np.zeros((len(starts), WC.OVER_MAX_WORD), dtype=np.uint8)
    for j in range(WC.OVER_MAX_WORD):
        m = lens > j
        rec[m, j] = data[starts[m] + j]
    keys = rec.view([("", np.uint8)] * WC.OVER_MAX_WORD).reshape(-1)
    assert len(np.unique(keys)) == len(starts)
    # documents begin on word starts; the splitter's words are these words; each is cacheable and needs the merge loop
    assert np.isin(offs[:-1], starts).all() and (np.diff(offs) > 0).all()
    sample = WC.overflow_sample(len(offs) - 1)
    assert sample[0] == 0 and sample[-1] == len(offs) - 2 and len(sample) >= (len(offs) - 1) // WC.OVER_SAMPLE
    words = []
    for d in sample:
        a, b = int(offs[d]), int(offs[d + 1])
        doc = data[a:b].tobytes()
        want = (starts[np.searchsorted(starts, a):np.searchsorted(starts, b)] - a).tolist()
        assert oracle_mod.split_words(doc) == want, d
        words += [doc[x:y] for x, y in zip(want, want[1:] + [len(doc)])]
    counts = WC.id_counts(orc, words)
    assert all(WC.cacheable(len(w), c) for w, c in zip(words, counts)), "a word of the sample is not a cacheable merge-loop word"
    # every sub-list: more than twice its capacity in word starts, counted by the kernel's block order
    per_shard = np.bincount(WC.shard_of_group(starts // WC.GROUP, n), minlength=WC.LIST_SHARDS)
    assert len(per_shard) == WC.LIST_SHARDS and int(per_shard.min()) >= 2 * WC.SHARD_CAP, int(per_shard.min())
    # the fresh batch shares no word with it, and learns
    fresh = WC.fresh_docs(3)
    assert sum(map(len, fresh)) >= WC.LARGE
    assert min(b - a for _d, a, b, _p in WC.word_spans(fresh)) > WC.OVER_MAX_WORD
    uniq = sorted({fresh[d][a:b] for d, a, b, _p in WC.word_spans(fresh)})
    assert len(uniq) > 1000 and all(WC.cacheable(len(w), c) for w, c in zip(uniq, WC.id_counts(orc, uniq)))


def _merge_loop_words(orc, words):
    return all(c >= 2 for c in WC.id_counts(orc, words))


def test_special_case(orc):
    c = WC.special_case(orc)
    docs, marks = c["docs"], c["marks"]
    A, B, C, D = c["words"]
    S, (left, right) = c["S"], c["halves"]
    assert sum(map(len, docs)) > WC.LARGE and sum(map(len, c["warm"])) >= WC.LARGE
    # the planted words: cacheable merge-loop words, one word each, all in the warm batch; the halves are other keys
    planted = [A, B, C, D, S, left, right]
    assert len(set(planted)) == 7 and left + right == S
    counts = WC.id_counts(orc, planted)
    assert all(WC.cacheable(len(w), n) for w, n in zip(planted, counts)), counts
    assert all(WC.is_one_word(w) for w in (A, B, C, D, S, left))
    warm_words = {c["warm"][d][a:b] for d, a, b, _p in WC.word_spans(c["warm"])}
    assert {A, B, C, D, S} <= warm_words and left not in warm_words and right not in warm_words
    # where the markers are, from the restatement's own scan
    blob, base, found = b"".join(docs), 0, []
    for doc in docs:
        found += [(base + a, base + b) for a, b, _i in SR.split(doc, {WC.EOT: WC.EOT_ID})]
        base += len(doc)
    at = {a for a, _b in found}
    n = len(WC.EOT)
    for name in ("behind A", "between", "inside S", "across an edge", "begins on an edge", "first in its document", "ends on an edge"):
        assert marks[name] in at, name
    p = marks["behind A"]
    assert blob[p - len(A):p] == A and blob[p + n:p + n + len(B)] == B           # directly behind a cached word, directly in front of one
    p = marks["between"]
    assert blob[p - len(B):p] == B and blob[p + n:p + n + len(C)] == C
    p = marks["inside S"]
    assert blob[p - len(left):p] == left and blob[p + n:p + n + len(right)] == right and blob[p + n + len(right):][:len(D)] == D
    p = marks["across an edge"]
    assert p < 2 * WC.TILE < p + n and p == 2 * WC.TILE - 5
    assert marks["begins on an edge"] == 4 * WC.TILE
    p = marks["ends on an edge"]
    assert p + n == 7 * WC.TILE and blob[p - len(D):p] == D
    offs = np.cumsum([0] + [len(d) for d in docs]).tolist()
    assert marks["first in its document"] in offs and marks["ends on an edge"] + n in offs
    # the pieces around the markers are cut into the planted words by the splitter
    piece_words = set()
    for doc in docs[:2]:
        for piece in SR.pieces(doc, {WC.EOT: WC.EOT_ID}):
            if isinstance(piece, bytes) and piece:
                piece_words |= {piece[a:b] for _d, a, b, _p in WC.word_spans([piece])}
    assert {A, B, C, D, left, right} <= piece_words


def test_preset_docs():
    import presplit_ref as R
    docs = WC.preset_docs()
    assert sum(map(len, docs)) > WC.LARGE and all(max(d) < 0x80 for d in docs)
    words = {p: {w for d in docs for w in R.words(d.decode("ascii"), p)} for p in WC.PRESETS}
    assert len({frozenset(w) for w in words.values()}) == 3, "two presets cut the batch alike"
    tab = {w for w in words["cl100k"] if w.startswith("\t") and len(w) > 4}
    assert tab and not tab & words["gpt2"] and tab <= words["qwen2"]
    dot = {w for w in words["cl100k"] if w.startswith(".") and len(w) > 4}
    assert dot and not dot & words["gpt2"]
    assert any(re.fullmatch(r" \d{7}", w) for w in words["gpt2"]) and not any(re.fullmatch(r" ?\d{4,}", w) for w in words["cl100k"])
    assert any(re.fullmatch(r"\d{3}", w) for w in words["cl100k"]) and all(len(w) == 1 for w in words["qwen2"] if w.isdigit())
    assert "'LL" in words["cl100k"] and "'LL" not in words["gpt2"] and "'ll" in words["gpt2"]
    # the stems are shared: the same bytes as a word under all three, and as part of other words under some
    stems = {w for w in words["gpt2"] if re.fullmatch(r" [a-z]{4,}", w)}
    assert len(stems) >= 150 and stems <= words["cl100k"] and stems <= words["qwen2"]


def test_exception_case(orc):
    c = WC.exception_case(orc)
    docs = c["docs"]
    assert sum(map(len, docs)) > WC.LARGE
    for kind, lo, hi, ids_lo, ids_hi in (("cached", 24, 30, 2, 16), ("long", 31, 45, 2, 99), ("many", 22, 30, 17, 99), ("short", 8, 9, 2, 16)):
        ws = c[kind]
        counts = WC.id_counts(orc, ws)
        assert all(lo <= len(w) <= hi and ids_lo <= n <= ids_hi for w, n in zip(ws, counts)), kind
        assert all(WC.is_one_word(w) for w in ws), kind
        assert all(WC.cacheable(len(w), n) == (kind in ("cached", "short")) for w, n in zip(ws, counts)), kind
    assert all(d[:1] != b" " and d[:1].isalpha() for d in docs)  # the first word gets the prefix
    tiles, n_tiles = WC.pending_per_tile(orc, docs)
    offs = np.cumsum([0] + [len(d) for d in docs])
    dd = c["dense_doc"]
    dense_doc_tiles = set(range(int(offs[dd]) // WC.TILE, int(offs[dd + 1]) // WC.TILE + 1))
    assert c["dense_tile"] in dense_doc_tiles
    kinds = {w: k for k in ("cached", "long", "many") for w in c[k]}
    mixed = 0
    for t in range(n_tiles - 1):
        ws = tiles.get(t, [])
        if t == c["dense_tile"]:
            # phase 6a's r0 loop takes a second trip; (the tile's last bytes begin one word of the other kinds)
            assert len(ws) > WC.ROUND and sum(w in c["short"] for w, _n in ws) >= len(ws) - 1 > WC.ROUND
        elif t not in dense_doc_tiles:
            assert 10 <= len(ws) <= 40, (t, len(ws))
            mixed += {kinds.get(w) for w, _n in ws} >= {"cached", "long", "many"}
    assert mixed >= 20  # cached words, words beyond the key and words beyond the result in one tile
    # ... and side by side
    spans = WC.word_spans(docs)
    pairs = {(kinds.get(docs[d][a:b]), kinds.get(docs[d2][a2:b2])) for (d, a, b, _p), (d2, a2, b2, _p2) in zip(spans, spans[1:]) if d == d2}
    assert {("cached", "long"), ("long", "cached"), ("cached", "many"), ("many", "cached")} <= pairs
    # document-first words in the same tiles as cached ones
    firsts = {int(o) // WC.TILE for o in offs[:-1]}
    assert len(firsts & set(tiles)) >= 10


def test_view_docs(orc):
    docs, first, last = WC.view_docs()
    assert sum(map(len, docs)) >= WC.LARGE
    spans = WC.word_spans(docs)
    ws = [docs[d][a:b] for d, a, b, _p in spans]
    assert ws[0] == first and ws[-1] == last and ws.count(first) >= 2 and ws.count(last) >= 2
    counts = WC.id_counts(orc, [first, last])
    assert all(WC.cacheable(len(w), n) for w, n in zip((first, last), counts))


def test_cjk_docs():
    docs = WC.cjk_docs()
    blob = b"".join(docs)
    assert WC.LARGE <= len(blob) <= 40 * WC.TILE
    # k_pre's sample (the 16 bytes 480 .. 495 of every tile, lead bytes of three-byte characters): far above one in eight
    hi = sum(1 for t in range(len(blob) // WC.TILE) for b in blob[t * WC.TILE + 480:t * WC.TILE + 496] if b >= 0xE0)
    assert hi * 8 * 8 >= 4 * (len(blob) // WC.TILE) * 16


def test_one_launch_case(orc, oracle_mod):
    c = WC.one_launch_case(orc)
    K, W30, W31, W3, W2 = c["K"], c["W30"], c["W31"], c["W3"], c["W2"]
    assert [len(w) for w in (K, W30, W31, W3, W2)] == [12, 30, 31, 3, 2]
    counts = WC.id_counts(orc, [K, W30, W31, W3, W2])
    assert [WC.cacheable(len(w), n) for w, n in zip((K, W30, W31, W3, W2), counts)] == [True, True, False, True, True], counts
    assert counts[2] >= 2
    assert sum(map(len, c["warm"])) >= WC.LARGE
    warm_words = {c["warm"][d][a:b] for d, a, b, _p in WC.word_spans(c["warm"])}
    assert {K, W30, W31, W3, W2} <= warm_words
    inputs = c["inputs"]
    planted = {}
    for name, (text, spans) in inputs.items():
        assert 1 <= len(text) <= WC.ONE_TILES * WC.TILE, name
        starts = oracle_mod.split_words(text) + [len(text)]
        for a, b in spans:
            assert a in starts and b in starts and not any(a < s < b for s in starts), name  # one word where it stands
            planted[name] = (a, b, text[a:b])
    full = WC.ONE_TILES * WC.TILE
    assert planted["at byte 0"][:2] == (0, 12)
    for name in ("ends at the last byte of four tiles", "30 bytes, ends at the last byte of four tiles"):
        assert planted[name][1] == full == len(inputs[name][0])
    for e in (1, 2, 3):
        a, b, w = planted["across the edge of tile %d" % e]
        assert a < e * WC.TILE < b and w == K
    assert inputs["the only word"][0] == K
    for n in (0, 2, 3, 5):
        text = inputs["30 bytes and %d behind" % n][0]
        assert text[:30] == W30 and len(text) == 30 + n and n < 6
    a, b, w = planted["30 bytes at the end of a tile and a half"]
    assert w == W30 and len(inputs["30 bytes at the end of a tile and a half"][0]) - a < 36  # nine dwords from the word's start pass the end
    assert [len(inputs["exactly %d bytes" % n][0]) for n in (2, 3, 30, 31)] == [2, 3, 30, 31]
