"""Every instantiation of the encode kernels on long words, under each of the three tails.

Which code encodes an exception word depends on the tables' kind (16- or 32-bit symbols, byte or character mode, rank ==
symbol order or not, items of several units: k_tiles' sixteen forms, k_exc_a<uint16_t / uint32_t>, k_exc_b<true / false>
and the five lists), on the tail the host enqueues (the one-launch k_tiles of the host form, k_tail_small for a batch of
at most 32 tiles and 4096 documents, k_exc_a .. k_finish beyond) and on the word's length in units.  tests/exc_cases.py
makes one vocabulary per kind and words on every limit in every position; tests/test_exc_cases_cpu.py checks those inputs
without a GPU.

The reference is the CPU oracle: every id, every output offset, every per-document status and the error word, bit-exact
(integer work, no tolerance), through helpers.compare.  Every [kind] test asserts from hutk_debug_exc_counts
(Context.exc_counts) the tail its batch got and the entries of the five lists, against exc_cases' plain restatement of
which list a word goes on -- a batch that went to another routine or another tail cannot pass for a test of this one.
Batches go in through the device entry point (the host form answers up to four tiles with the one-launch kernel), with
k_tiles in front (hutk_debug_tile_kernel says 0) unless the test says otherwise.  Needs a real MI355X."""
import numpy as np
import pytest

import exc_cases as X
import helpers as H

pytestmark = pytest.mark.gpu

KIND_TAGS = list(X.KINDS)
SWITCHES = ("HUTK_PTILES", "HUTK_PTILES_MIN_TILES", "HUTK_NO_SEAM", "HUTK_NO_SEAM2", "HUTK_NO_WORD_TABLE", "HUTK_NO_LONG_WORD_TABLE",
            "HUTK_ONE_SHOT")  # (HUTK_ONE_SHOT is read once per process: test_one_launch asserts the path from the diagnostic)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


@pytest.fixture(scope="module")
def made(tmp_path_factory, oracle_mod):
    """tag -> (Kind, GPU context, oracle), each made once."""
    from hutoken_amd import _capi
    tmp = tmp_path_factory.mktemp("exck")
    cache = {}

    def get(tag):
        if tag not in cache:
            k = X.kind(tag, tmp)
            ctx = _capi.Context(k.vp, k.sp, k.prefix, k.is_byte, device=0, merges_path=k.mp)
            cache[tag] = (k, ctx, X.oracle(k, oracle_mod))
        return cache[tag]
    yield get
    for _k, ctx, _o in cache.values():
        ctx.close()


def _encoder(ctx, log, tile_kernel=0):
    """-> encode(data, offsets) for H.compare: the device form with `tile_kernel` in front, what it wrote and, appended to
    `log`, where the batch's exception words went."""
    def encode(data, offs):
        assert ctx.tile_kernel(int(offs[-1])) == tile_kernel, "another tile kernel would be in front"
        got = H.DeviceBatch(ctx, data, offs).run()
        log.append((ctx.exc_counts(), got))
        return got
    return encode


def _check_lists(k, docs, counts, tail, sw):
    """The diagnostic's numbers for the batch `docs` against the restatement; -> the restatement's listed words."""
    want, unknown, listed = X.list_counts(k, docs, k.seams, sw)
    assert counts["tail"] == tail, counts
    assert counts["has_multi"] == k.multi, counts
    got = counts["lists"]
    assert unknown == 0, (k.tag, unknown)  # (the restatement can tell every word's list: tests/test_exc_cases_cpu.py)
    assert got == want, (k.tag, got, want)
    if k.multi:
        assert got[4] == counts["exc"], counts  # every exception word is expanded by d_exc
    assert counts["exc"] >= sum(got)
    fast = (not k.sym32) and k.rank_is_sym and not k.multi
    quad = fast or (k.is_byte and k.rank_is_sym and not k.multi)
    if not fast:
        assert got[2] == got[3] == 0
    if not quad:
        assert got[0] == got[1] == 0
    return listed


_full, _small = {}, {}


def _run_full(made, oracle_mod, tag):
    """The full batch of a kind: compared with the oracle and its lists checked once; -> (documents, ids, offsets)."""
    if tag not in _full:
        k, ctx, orc = made(tag)
        docs, log = X.full_docs(k), []
        assert X.tiles_of(docs) > 4 * X.SMALL_TILES
        H.compare(ctx, orc, docs, "full " + tag, encode=_encoder(ctx, log))
        counts, got = log[-1]
        listed = _check_lists(k, docs, counts, 0, oracle_mod.split_words)
        used = {X.list_of(k, n) for n in (100, 200, 400, 800, 1500)}
        assert all(counts["lists"][li] >= 10 for li in used), counts
        _full[tag] = (docs, got[0], got[1], listed)
    return _full[tag]


def _run_small(made, oracle_mod, tag):
    """Every small batch of a kind; -> [(documents, ids, offsets, counts)]."""
    if tag not in _small:
        k, ctx, orc = made(tag)
        batches, left_out = X.small_batches(X.full_docs(k))
        assert not left_out
        out = []
        for i, docs in enumerate(batches):
            assert 5 <= X.tiles_of(docs) <= X.SMALL_TILES and len(docs) <= X.SMALL_DOCS
            log = []
            H.compare(ctx, orc, docs, "small %s #%d" % (tag, i), encode=_encoder(ctx, log))
            counts, got = log[-1]
            listed = _check_lists(k, docs, counts, 1, oracle_mod.split_words)
            out.append((docs, got[0], got[1], counts, listed))
        _small[tag] = out
    return _small[tag]


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_full_tail(made, oracle_mod, tag):
    """All documents of the kind in one batch, well past 32 tiles: k_exc_a, k_exc_b, k_scan and k_finish."""
    _run_full(made, oracle_mod, tag)


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_small_tail(made, oracle_mod, tag):
    """The same documents in consecutive batches of 5..32 tiles: k_tail_small, one wavefront, every stage in one LDS array,
    d_exc with 1024 units of LDS (1025..2046 units merge in HBM here and in LDS under k_exc_b<true>).  At least one batch
    has entries on every list the kind uses at once, and one a wave-list word of 1025..2046 units."""
    k = made(tag)[0]
    runs = _run_small(made, oracle_mod, tag)
    used = {X.list_of(k, n) for n in (100, 200, 400, 800, 1500)}
    assert sum(all(c["lists"][li] > 0 for li in used) for _d, _i, _o, c, _l in runs) >= 1
    assert sum(any(li == 4 and 1025 <= X.units(k, docs[d], a, b) <= 2046 for d, a, b, li in listed)
               for docs, _i, _o, _c, listed in runs) >= 1


@pytest.mark.parametrize("tag", X.ONE_LAUNCH_KINDS)
def test_one_launch(made, oracle_mod, tag):
    """Each limit word of up to 3800 bytes alone, or with one short neighbour, through the host form: at most four tiles
    and no item of several units is what one_shot_takes asks, so k_tiles<..., ONE> runs the whole pipeline (the diagnostic
    says tail 2) or, for a batch with exception words, hands on to k_tail_small (tail 3).  A batch that fell back to the
    three launches would say 0 or 1.  The lists are the restatement's, as under the other tails."""
    k, ctx, orc = made(tag)
    assert not k.multi
    batches = X.one_launch_batches(k)
    assert len(batches) > 50
    sw = oracle_mod.split_words
    tails = set()
    for i, docs in enumerate(batches):
        assert 1 <= X.tiles_of(docs) <= X.ONE_TILES
        H.compare(ctx, orc, docs, "one-launch %s #%d" % (tag, i))
        counts = ctx.exc_counts()
        has_exc = any(X.is_exception_word(k, d, a, b) for d in docs for a, b in X.gpu_words(d, k.seams, sw))
        _check_lists(k, docs, counts, 3 if has_exc else 2, sw)
        assert (counts["exc"] > 0) == has_exc, counts
        tails.add(counts["tail"])
    assert tails == {2, 3}


@pytest.mark.parametrize("tag", KIND_TAGS)
def test_full_and_small_tails_agree(made, oracle_mod, tag):
    """The ids of a word are the same whichever tail encoded it: three documents of one long word per list, by name."""
    k = made(tag)[0]
    docs, ids, oo, listed = _run_full(made, oracle_mod, tag)
    runs = _run_small(made, oracle_mod, tag)
    where = {}
    for bi, (bdocs, _i, _o, _c, _l) in enumerate(runs):
        for di, d in enumerate(bdocs):
            where.setdefault(d, (bi, di))
    picked = {}
    for d, a, b, li in listed:
        if a == 0 and b == len(docs[d]) and len(picked.setdefault(li, [])) < 3:
            picked[li].append(d)
    used = {X.list_of(k, n) for n in (100, 200, 400, 800, 1500)}
    assert set(picked) >= used and all(len(v) == 3 for v in picked.values()), {li: len(v) for li, v in picked.items()}
    for li, ds in picked.items():
        for d in ds:
            bi, di = where[docs[d]]
            _bd, sids, soo, counts, _l = runs[bi]
            assert counts["tail"] == 1
            full_ids, small_ids = ids[oo[d]:oo[d + 1]], sids[soo[di]:soo[di + 1]]
            assert np.array_equal(full_ids, small_ids), "list %d, word %r: the tails differ" % (li, docs[d][:200])


@pytest.mark.parametrize("tag", X.GIANT_KINDS)
def test_giant_words_of_the_other_kinds(made, oracle_mod, tag):
    """Words of 65 536 and 65 537 units, where bpe_wave_big's chunk steps from 64 to 128 units, under the kinds that do not
    have the fast routines (tests/test_gpu_parity.py::test_giant_words has them for the GPT-2 vocabulary)."""
    k, ctx, orc = made(tag)
    docs, log = X.giant_docs(k), []
    H.compare(ctx, orc, docs, "giant " + tag, encode=_encoder(ctx, log))
    counts = log[-1][0]
    listed = _check_lists(k, docs, counts, 0, oracle_mod.split_words)
    assert sorted(X.units(k, docs[d], a, b) for d, a, b, li in listed if li == 4)[-2:] == list(X.GIANT)


def test_ptiles_in_front(made, oracle_mod, monkeypatch):
    """The full batch of B16 behind the persistent tile kernel (HUTK_PTILES=1, HUTK_PTILES_MIN_TILES=1: ptiles_takes wants
    16-bit symbols in byte mode): the same lists, the same ids.  A 32-bit kind gets k_tiles under the same switches."""
    monkeypatch.setenv("HUTK_PTILES", "1")
    monkeypatch.setenv("HUTK_PTILES_MIN_TILES", "1")
    k, ctx, orc = made("B16")
    docs, log = X.full_docs(k), []
    H.compare(ctx, orc, docs, "ptiles B16", encode=_encoder(ctx, log, tile_kernel=1))
    _check_lists(k, docs, log[-1][0], 0, oracle_mod.split_words)
    k32, ctx32, _o = made("B32")
    assert ctx32.tile_kernel(sum(len(d) for d in X.full_docs(k32))) == 0


# ---- 32-bit tables behind the other encoders: the vocabularies the cl100k / qwen2 presets exist for are all of this kind ----

WHOLE = "(.|\n)+"  # the whole-document pattern of tests/test_regex_path.py: the oracle encodes a document as ONE word


@pytest.fixture(scope="module")
def lc_ctype():
    import json
    import locale
    import os
    with open(os.path.join(H.GOLDEN_DIR, "g9_regex_path.json")) as f:
        want = json.load(f)["lc_ctype"]
    if locale.setlocale(locale.LC_CTYPE, None) != want:
        pytest.skip("POSIX regex matching depends on LC_CTYPE; the whole-document pattern was checked under " + want)


def _limit_texts(k, forms, up_to):
    return [d.decode("utf-8") for d, form, u, _c in X.limit_docs(k) if form in forms and u <= up_to]


def _b32_module(made, pretokenizer=None):
    """The module-level API initialised with B32's files -> (hutoken_amd, Kind, oracle)."""
    import hutoken_amd as hutoken
    k, _ctx, orc = made("B32")
    hutoken.initialize(k.vp, k.sp, is_byte_encoder=True, pretokenizer=pretokenizer)
    assert hutoken.context().table_stats()["n_sym"] >= 65520
    return hutoken, k, orc


def test_32_bit_symbols_behind_the_cl100k_preset(made, oracle_mod, lc_ctype):
    """encode_packed_device with pretokenizer="cl100k" on B32: the ids are the oracle's of the restatement's words
    (tests/presplit_ref.py), each encoded as a document of its own, as tests/test_gpu_presplit.py builds them."""
    import presplit_cases as PC
    import presplit_ref as R
    import torch
    hutoken, k, _orc = _b32_module(made, "cl100k")
    assert hutoken.context().pretokenizer == R.PRESETS.index("cl100k")
    texts = _limit_texts(k, ("alone", "behind-short", "short-behind"), 2049)
    texts += [t.replace("\0", "?") for t in PC.seeded_texts(60, 47, 20, 200)] + ["", " ", "we'll've  \t done 1234567", "x" * 300]
    assert max(len(t) for t in texts) > 2000
    orc = oracle_mod.Oracle(k.vp, k.sp, None, True, pattern=WHOLE)
    words = [[w.encode("utf-8") for w in R.words(t, "cl100k")] for t in texts]
    assert max(len(w) for ws in words for w in ws) >= 2049  # a long run of letters stays one word under the preset
    flat = [w for ws in words for w in ws]
    ids_o, oo_o, _st = orc.encode_packed(*oracle_mod.pack(flat), 4)
    want, at = [], 0
    for ws in words:
        want.append(ids_o[oo_o[at]:oo_o[at + len(ws)]].tolist())
        at += len(ws)
    dev = torch.device("cuda", 0)
    data, offs = oracle_mod.pack(texts)
    d_bytes, d_offs = torch.from_numpy(np.array(data, copy=True)).to(dev), torch.from_numpy(np.array(offs, copy=True)).to(dev)
    ids, oo = hutoken.encode_packed_device(d_bytes, d_offs, check=True)
    counts = hutoken.context().exc_counts()
    assert counts["tail"] == 0 and counts["lists"][0] > 0 and counts["lists"][1] > 0 and counts["lists"][4] > 0, counts
    assert counts["lists"][2] == counts["lists"][3] == 0
    oo = oo.tolist()
    ids = ids[:oo[-1]].tolist()
    bad = [i for i in range(len(texts)) if ids[oo[i]:oo[i + 1]] != want[i]]
    assert not bad, (bad[:5], texts[bad[0]][:200], ids[oo[bad[0]]:oo[bad[0] + 1]][:20], want[bad[0]][:20])
    orc.close()


def test_32_bit_symbols_with_special_tokens(made, oracle_mod):
    """batch_encode_special on B32 with two markers, one of them cutting a word of 300 units in two; the reference is
    tests/specials_ref.py over the oracle.  The pieces between the markers are the documents of the batch the encode
    kernels get: well past 32 tiles (the full tail), and the lists hold the restatement's counts over those pieces."""
    import random
    import specials_ref as SR
    hutoken, k, orc = _b32_module(made)
    specials = {"<|cut|>": 80001, "<|end|>": 80002}
    raw_specials = {s.encode(): i for s, i in specials.items()}
    hutoken.set_special_tokens(specials)
    try:
        rng = random.Random(77)
        w300 = X.word(k, rng, 300).decode()
        texts = [w300[:150] + "<|cut|>" + w300[150:], w300 + "<|end|>", "<|end|>" + w300 + " ab<|cut|>",
                 X.word(k, rng, 1030).decode() + "<|cut|><|end|>" + X.word(k, rng, 129).decode(), "no marker " + w300]
        texts += [t[: len(t) // 2] + "<|cut|>" + t[len(t) // 2:] for t in _limit_texts(k, ("alone", "behind-short", "short-behind"), 3000)]
        data, offs = oracle_mod.pack(texts)
        ids_o, oo_o, st_o, matches = SR.encode(orc, data, offs, raw_specials)
        assert matches >= len(texts) and (st_o == 0).all()
        want = [ids_o[oo_o[i]:oo_o[i + 1]].tolist() for i in range(len(texts))]
        got = hutoken.batch_encode_special(texts)
        counts = hutoken.context().exc_counts()
        pieces = [p for t in texts for p in SR.pieces(t.encode("utf-8"), raw_specials) if isinstance(p, bytes)]
        assert X.tiles_of(pieces) > X.SMALL_TILES + 4
        _check_lists(k, pieces, counts, 0, oracle_mod.split_words)
        assert counts["lists"][0] > 0 and counts["lists"][1] > 0 and counts["lists"][4] > 0, counts
        bad = [i for i in range(len(texts)) if got[i] != want[i]]
        assert not bad, (bad[:5], texts[bad[0]][:200], got[bad[0]][:20], want[bad[0]][:20])
        assert hutoken.encode_special(texts[0]) == want[0]
    finally:
        hutoken.set_special_tokens(None)


def test_32_bit_symbols_with_token_offsets(made, oracle_mod):
    """batch_encode_with_offsets on B32's limit words: the oracle's ids, spans that tile each document, and the decoding
    of each id is the slice its span names.  The batch is well past 32 tiles (the full tail) and its lists hold the
    restatement's counts."""
    hutoken, k, orc = _b32_module(made)
    texts = _limit_texts(k, ("alone", "behind-short", "short-behind"), 3000) + _limit_texts(k, ("space-first",), 3000)[-3:]
    ids_b, spans_b = hutoken.batch_encode_with_offsets(texts, unit="byte")
    counts = hutoken.context().exc_counts()
    docs = [t.encode("utf-8") for t in texts]
    assert X.tiles_of(docs) > X.SMALL_TILES
    _check_lists(k, docs, counts, 0, oracle_mod.split_words)
    assert counts["lists"][0] > 0 and counts["lists"][1] > 0 and counts["lists"][4] > 0, counts
    ids_o, oo_o, _st = orc.encode_packed(*oracle_mod.pack(texts), 4)
    for n, (t, ids, spans) in enumerate(zip(texts, ids_b, spans_b)):
        raw = t.encode("utf-8")
        assert ids == ids_o[oo_o[n]:oo_o[n + 1]].tolist(), t[:200]
        assert [a for a, _b in spans] == [0] + [b for _a, b in spans[:-1]] and spans[-1][1] == len(raw)
        if len(raw) <= 300 or n % 7 == 0:
            assert [hutoken.decode([i]) for i in ids] == [raw[a:b].decode("utf-8") for a, b in spans], t[:200]


def test_byte_fallback_on_32_bit_character_tables(made, oracle_mod):
    """C32's limit words with one character in twenty replaced by one the vocabulary does not hold: the expected ids are
    tests/fallback_ref.py's expansion of the ORACLE's plain ids (every -1 becomes the table ids of its character's bytes)."""
    import random
    import fallback_ref as F
    import spans_ref as S
    k, ctx, orc = made("C32")
    table, found = ctx.find_byte_tokens()
    assert found == 256
    ctx.set_byte_fallback(table)
    try:
        rng = random.Random(78)
        unknown = {1: "ßž", 2: "ßž", 3: "語文"}
        docs = []
        for d, form, u, _c in X.limit_docs(k):
            if form in ("alone", "behind-short", "long-behind"):
                s = list(d.decode("utf-8"))
                for i in range(len(s)):
                    if s[i] != " " and rng.random() < 0.05:
                        s[i] = rng.choice(unknown[len(s[i].encode("utf-8"))])
                docs.append("".join(s).encode("utf-8"))
        data, offs = oracle_mod.pack(docs)
        assert X.tiles_of(docs) > X.SMALL_TILES
        ids_o, oo_o, st_o = orc.encode_packed(data, offs, 4)
        assert (st_o == 0).all() and 0.02 < float((ids_o == -1).mean()) < 0.5
        want, woo, mism = F.encode(S.TokenText(orc), data, offs, ids_o, oo_o, False, table)
        assert not mism.any() and (want >= 0).all()
        got, goo, gst, rc = ctx.encode_fallback_packed(data, offs)
        counts = ctx.exc_counts()
        assert counts["tail"] == 0 and counts["lists"][:4] == [0, 0, 0, 0] and counts["lists"][4] >= 100, counts
        assert rc == 0 and np.array_equal(goo, woo) and (gst == 0).all()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    finally:
        ctx.set_byte_fallback(None)
