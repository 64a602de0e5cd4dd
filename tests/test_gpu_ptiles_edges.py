"""The persistent tile kernel (csrc/hutk_ptiles.hip, k_ptiles) on the small and odd batches where it can go wrong.

By default the kernel is given batches of at least four tiles per workgroup (about 1 MB), so the edge tests written for
k_tiles never reach it.  Here HUTK_PTILES_MIN_TILES=1 lifts that limit and HUTK_PTILES=1 forces the kernel (fixture
`forced`), or leaves the choice to the device (fixture `auto`: both kernels are enqueued, Workspace::select).  Every test
first asserts what hutk_debug_tile_kernel reports for its batch -- 1 forced, 2 auto, 0 for a vocabulary the kernel refuses
-- so that a batch which silently went to k_tiles cannot pass for a test of k_ptiles.

The reference is the CPU oracle: every id, every output offset, every per-document status and the error word, bit-exact
(integer work, no tolerance).  Batches go in through the DEVICE entry point (hutk_encode_batch_device): the host form
answers a batch of up to four tiles with a one-launch k_tiles that never asks for the persistent kernel.  Where it says
"twin", k_tiles (HUTK_PTILES=0) encodes the same device buffers as well and ids, offsets, status and error word of the
two must be equal.

Constants cited below: TILE_BYTES = 960, LOOKBACK = 16, HALO = 64, LANE_MAX_UNITS = 32, LANE_MAX_BYTES = 63 (hutk_device.h);
PT_SLOTS = 30, PT_QCAP = 2048, PT_STAGE = 256, PT_ROOM_AHEAD = 64, PT_WAVES = 16 (hutk_ptiles.hip).  G is the kernel's
grid: the compute units rounded down to a multiple of 8 (pt_grid()), read from the device.  Needs a real MI355X."""
import os
import random

import numpy as np
import pytest

import helpers as H
from helpers import DeviceBatch as _Batch, device_encoder as _encoder, env_switches as _env, side_stream as _stream

pytestmark = pytest.mark.gpu

TILE, LOOKBACK, HALO = 960, 16, 64
PT_SLOTS, PT_QCAP, PT_STAGE, PT_ROOM_AHEAD = 30, 2048, 256, 64
E_DEVICE, E_NUL_BYTE, E_WORD_TOO_LARGE = 5, 8, 9
SWITCHES = ("HUTK_PTILES", "HUTK_PTILES_MIN_TILES", "HUTK_NO_SEAM", "HUTK_NO_SEAM2", "HUTK_NO_WORD_TABLE")
TAKEN = ("VG", "VGM", "VC", "RB")  # contexts the kernel takes; "RX" is the random vocabulary it refuses


@pytest.fixture
def forced(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HUTK_PTILES", "1")
    monkeypatch.setenv("HUTK_PTILES_MIN_TILES", "1")


@pytest.fixture
def auto(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HUTK_PTILES_MIN_TILES", "1")


@pytest.fixture(scope="module")
def vocabs(tmp_path_factory):
    """name -> (vocabulary file, special file, merges file or None).  RB: random_byte_vocab(1) with 500 merges, which the
    kernel takes; RX: random_byte_vocab(3) with duplicate ids (rank_is_sym == 0), which it refuses."""
    from hutoken_amd import data
    tmp = tmp_path_factory.mktemp("ptv")
    out = {}
    for name in ("VG", "VC"):
        vp, sp, kw = data.vocab_files(name)
        assert kw["is_byte_encoder"] and kw["prefix"] is None
        out[name] = (vp, sp, None)
    out["VGM"] = out["VG"][:2] + (data.merges_file("VG"),)
    for name, seed, dup in (("RB", 1, False), ("RX", 3, True)):
        ents, special = H.random_byte_vocab(seed, n_merges=500, dup_ids=dup)
        out[name] = H.write_vocab(tmp, name, ents, special) + (None,)
    return out


_made = {}


def _pair(vocabs, oracle_mod, name, **switches):
    """-> (GPU context, oracle), made once per module and per set of creation-time switches (HUTK_NO_SEAM, HUTK_NO_SEAM2,
    HUTK_NO_WORD_TABLE)."""
    key = (name,) + tuple(sorted(switches.items()))
    if key not in _made:
        from hutoken_amd import _capi
        vp, sp, mp = vocabs[name]
        with _env(**switches):
            ctx = _capi.Context(vp, sp, None, True, device=0, merges_path=mp)
        if ("o", name) not in _made:
            _made[("o", name)] = oracle_mod.Oracle(vp, sp, None, True, merges_path=mp)
        _made[key] = (ctx, _made[("o", name)])
    return _made[key]


def _seams_on(ctx):
    """Was the context made with the seam map in use?  (Only then does the automatic mode enqueue both kernels.)"""
    with _env(HUTK_PTILES=None, HUTK_PTILES_MIN_TILES="1"):
        return ctx.tile_kernel(TILE) == 2


def _grid():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


def _check(ctx, orc, docs, tag, want=1, twin=True, want_rc=0):
    H.compare(ctx, orc, docs, tag, encode=_encoder(ctx, want, twin), want_rc=want_rc)


# ---- inputs ------------------------------------------------------------------------------------------------

_text_blob = None


def _text(n, at=0):
    """n bytes of ordinary mixed text (random_text, seeded), from byte `at` of a blob made once."""
    global _text_blob
    if _text_blob is None:
        rng = random.Random(41)
        _text_blob = "".join(H.random_text(rng, max_words=30) for _ in range(600)).encode("utf-8").replace(b"\0", b"")
    assert at + n <= len(_text_blob)
    return _text_blob[at:at + n]


SIZES = [1, 15, 16, 17, 959, 960, 961, 976, 1919, 1920, 1921]
SPLITS = [0, 1, 959, 960, 961]


def _partial_window_batches():
    """Item 1: one document of each size, and the same split into two documents at each offset."""
    out = []
    for k, n in enumerate(SIZES):
        t = _text(n, 37 * k)
        out.append(("%d" % n, [t]))
        out += [("%d split at %d" % (n, c), [t[:c], t[c:]]) for c in SPLITS if c <= n]
    return out


def _cut_to_tiles(data, offs, n_tiles, slack=400):
    """The first documents of (data, offs), the last one cut short, so that the batch is n_tiles tiles less `slack` bytes."""
    nb = n_tiles * TILE - slack
    assert (n_tiles - 1) * TILE < nb <= int(offs[-1]), (n_tiles, int(offs[-1]))
    raw = data.tobytes()[:nb]
    cuts = [int(x) for x in offs if x < nb] + [nb]
    return [raw[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _c3_tiles(n_tiles):
    from hutoken_amd import synth
    d, o = synth.corpus("C3", 200 + n_tiles * 3)
    return _cut_to_tiles(d, o, n_tiles)


def _cjk_tiles(gen, n_tiles):
    from hutoken_amd import synth
    d, o = getattr(synth, gen)(8 + n_tiles * 3)
    return _cut_to_tiles(d, o, n_tiles)


def _document_batches():
    """Item 6 -> [(tag, documents)]."""
    rng = random.Random(66)
    one = [bytes([rng.choice(b"ab \n.1x")]) for _ in range(3000)]
    out = []
    for k in (65, 128):  # that many one-byte documents at the start of a tile, text behind them, twice
        out.append(("%d one-byte documents in a tile" % k,
                    one[:k] + [_text(TILE - k, 5)] + one[k:2 * k] + [_text(TILE - k + 300, 900)] + one[:3]))
    out.append(("960 one-byte documents: a whole tile", one[:TILE] + [_text(500)]))
    out.append(("2000 one-byte documents over tile limits", one[:2000]))
    t = _text(3 * TILE, 100)
    out.append(("empty documents at the start", [b""] * 70 + [t[:1000], t[1000:]]))
    out.append(("empty documents on a tile limit", [t[:TILE]] + [b""] * 130 + [t[TILE:TILE + 5]] + [b""] * 3 + [t[TILE + 5:]]))
    out.append(("empty documents just behind a tile limit", [t[:TILE + 1]] + [b""] * 65 + [t[TILE + 1:]]))
    out.append(("empty documents in the look-back", [t[:TILE - LOOKBACK]] + [b""] * 65 + [t[TILE - LOOKBACK:TILE - 1]] + [b""] * 64 + [t[TILE - 1:]]))
    out.append(("empty documents at the end", [t[:2 * TILE]] + [b""] * 200))
    out.append(("empty documents at the end, behind a partial tile", [t[:2 * TILE + 7]] + [b""] * 65))
    out.append(("only the last document is not empty", [b""] * 300 + [t[:1500]]))
    out.append(("only the last document is not empty, one byte", [b""] * 64 + [b"a"]))
    out.append(("ragged", H.ragged_docs()))
    return out


# ---- 1. tile count and partial windows -------------------------------------------------------------------------

@pytest.mark.parametrize("name", TAKEN)
def test_partial_windows(forced, vocabs, oracle_mod, name):
    """One document of 1 .. 1921 bytes, whole and split in two at 0, 1, 959, 960, 961: batches of one to three tiles (TILE_BYTES
    = 960).  The first tile's window begins LOOKBACK = 16 bytes before the data and the last one ends short of its HALO, so
    both are staged byte by byte (pf_whole false); all but one to three of the G workgroups have no tile (n_my == 0); 961 and
    976 leave a last tile shorter than or as long as the look-back.  Twin."""
    ctx, orc = _pair(vocabs, oracle_mod, name)
    for tag, docs in _partial_window_batches():
        _check(ctx, orc, docs, "%s %s" % (name, tag))


# ---- 2. range arithmetic ---------------------------------------------------------------------------------------

def test_tiles_per_workgroup(forced, vocabs, oracle_mod):
    """G - 1, G, G + 1, 2G - 1 and 2G + 1 tiles of ordinary text (corpus C3): per = ceil(n_tiles / G) tiles per workgroup; at
    G + 1 half of the workgroups get two tiles and the others must clamp their range to n_tiles.  Twin."""
    G = _grid()
    ctx, orc = _pair(vocabs, oracle_mod, "VG")
    for n in (G - 1, G, G + 1, 2 * G - 1, 2 * G + 1):
        _check(ctx, orc, _c3_tiles(n), "%d tiles (G = %d)" % (n, G))


# ---- 3. slot recycling and ring wrap ---------------------------------------------------------------------------

def _merge_lines(rng, n_bytes, lengths):
    """Documents (lines of a few hundred bytes) of random words over eight rare letters, each line of words of one of the
    `lengths` (lo, hi): n_bytes in all."""
    docs, size = [], 0
    while size < n_bytes:
        lo, hi = rng.choice(lengths)
        docs.append(H.merge_loop_words(rng, rng.randint(20, 90), lo, hi))
        size += len(docs[-1])
    docs[-1] = docs[-1][:len(docs[-1]) - (size - n_bytes)]
    return docs


MERGE_CONTEXTS = [("RB", {}), ("RB", {"HUTK_NO_WORD_TABLE": "1"}), ("VG", {})]
MERGE_IDS = ["RB", "RB-no-word-table", "VG"]


@pytest.mark.parametrize("name,switches", MERGE_CONTEXTS, ids=MERGE_IDS)
def test_merge_queue_wraps(forced, vocabs, oracle_mod, name, switches):
    """8 G + 1 tiles of two- and three-letter words that nearly all need the merge loop (about 270 a tile): nine tiles per
    workgroup put more than PT_QCAP = 2048 entries through its ring, which wraps, and thirty slots of such tiles fill it, so
    that front ends wait for room (q_room).  The random vocabulary with the whole-word table and without it
    (HUTK_NO_WORD_TABLE=1: every word of two bytes and more is a merge word, though few of its letters merge), and VG, in which
    they do merge.  Twin."""
    G = _grid()
    ctx, orc = _pair(vocabs, oracle_mod, name, **switches)
    docs = _merge_lines(random.Random(8), (8 * G + 1) * TILE - 300, [(2, 3)])
    blob = b"".join(docs)
    assert (len(blob) + TILE - 1) // TILE == 8 * G + 1
    per_tile = min(blob[t * TILE:(t + 1) * TILE].count(b" ") for t in range(8 * G))
    assert 9 * per_tile > PT_QCAP, per_tile  # (every space begins a word of three or four bytes)
    _check(ctx, orc, docs, "8G+1 tiles of short merge words")


@pytest.mark.parametrize("name,switches", MERGE_CONTEXTS, ids=MERGE_IDS)
def test_slots_are_reused(forced, vocabs, oracle_mod, name, switches):
    """(PT_SLOTS + 2) G tiles, 32 a workgroup: more than its PT_SLOTS = 30 slots, so slots are given back by epilogues and
    taken again.  Words of 2-3 and of 10-14 rare letters, half the lines each.  Every id against the oracle (a few seconds
    for these 7.5 MB on eight threads), and twin."""
    G = _grid()
    ctx, orc = _pair(vocabs, oracle_mod, name, **switches)
    want = (PT_SLOTS + 2) * G * TILE - 300
    docs = _merge_lines(random.Random(30), want, [(2, 3), (10, 14)])
    assert (want + TILE - 1) // TILE == (PT_SLOTS + 2) * G
    _check(ctx, orc, docs, "32G tiles of merge words")


# ---- 4. staging limits inside one tile -------------------------------------------------------------------------

@pytest.mark.parametrize("name,switches", MERGE_CONTEXTS, ids=MERGE_IDS)
def test_staging_limits_of_a_tile(forced, vocabs, oracle_mod, name, switches):
    """More word starts than a front end stages at a time (PT_STAGE = 256): "\\tab" and " ab" back to back are 320 words of
    several bytes per tile.  More merge-loop words than the queue room a front end reserves before it knows them
    (PT_ROOM_AHEAD = 64): tiles of exactly 63, 64, 65, 66 and 128 three-byte words among newlines -- without the whole-word
    table each of them is a merge word, so the counts are exact there.  Tiles where every byte is a word, and the
    documents of test_dense_word_tiles.  Twin."""
    ctx, orc = _pair(vocabs, oracle_mod, name, **switches)
    docs = [b"\tab" * 1000, b" ab" * 1000, b"ab" + b"\tab" * 700 + b" ab" * 700]
    for k in (63, 64, 65, 66, 128):
        tile = b" qx" * k + b"\n" * (TILE - 3 * k)
        rng = random.Random(k)
        other = b"".join(b" " + bytes(rng.choice(b"qxzjkvwy") for _ in range(2)) for _ in range(k))
        docs.append(tile + other + b"\n" * (TILE - 3 * k) + tile[:500])
    _check(ctx, orc, docs, "stage and room")
    for k, doc in enumerate(docs):  # ... and each alone: its tiles at the start of a batch
        _check(ctx, orc, [doc], "stage and room, document %d alone" % k)
    _check(ctx, orc, H.dense_word_docs(), "dense")
    _check(ctx, orc, [bytes([b]) for b in range(1, 256)] * 8, "one-byte-docs")


# ---- 5. lane limit and the halo --------------------------------------------------------------------------------

WORD_LENGTHS = [16, 17, 31, 32, 33, 62, 63, 64, 65]
WORD_STARTS = [0, 895, 896, 927, 928, 958, 959]


def _placed_words(rng):
    """-> (one batch with every (length, start, what follows), [a batch that ends with the word, per (length, start)])."""
    def word(n):
        return bytes(rng.choice(b"etaoinshrdlu") for _ in range(n))

    def lead(size, p):  # newlines (one-byte words) up to the next offset that is p into a tile, at least one
        pad = (p - size) % TILE
        return b"\n" * (pad if pad or size == 0 else TILE)
    docs, size, alone = [], 0, []
    for n in WORD_LENGTHS:
        for p in WORD_STARTS:
            for behind in (b" x", b" " + word(40), None):
                doc = lead(size, p) + word(n)
                assert (size + len(doc) - n) % TILE == p
                if behind is None:  # the document ends with the word
                    docs.append(doc)
                    size += len(doc)
                    doc = b""
                else:
                    doc += behind
                doc += b" tail"
                docs.append(doc)
                size += len(doc)
            alone.append([b"\n" * p + word(n)])
            alone.append([b"a\n" * 480, b"\n" * p + word(n)])  # ... in the batch's second tile, at a document's start when p == 0
    return docs, alone


@pytest.mark.parametrize("name", ["RB", "VG"])
def test_words_at_the_lane_limit_and_the_halo(forced, vocabs, oracle_mod, name):
    """Words of 16 .. 65 letters that start 0, 895, 896, 927, 928, 958 and 959 bytes into a tile.  16 and 17: the 16-byte key
    masks of the whole-word probe (s_mask); 31 .. 33: LANE_MAX_UNITS = 32, the longest word a lane merges; 62 .. 65:
    LANE_MAX_BYTES = 63, beyond which the front end sees no end.  From 895 a word of 65 ends on the tile limit; from 959 one of
    65 ends on the last classified position (TILE_BYTES + HALO = 1024) and anything longer is not visible: those are
    exception words whose records (excm, exc_first, tile_first_start) k_ptiles writes for the kernels behind it.  Behind
    each word: a short word, a long word, the document's end, the batch's end.  Twin."""
    ctx, orc = _pair(vocabs, oracle_mod, name)
    docs, alone = _placed_words(random.Random(5))
    _check(ctx, orc, docs, "placed words")
    for k, batch in enumerate(alone):
        _check(ctx, orc, batch, "word %d of %d bytes ends the batch" % (k, len(batch[-1])))


@pytest.mark.parametrize("name", ["RB", "VG"])
def test_words_that_end_in_later_tiles(forced, vocabs, oracle_mod, name):
    """The documents of test_word_ends_in_later_tiles and test_long_words_exception_path (tests/helpers.py), the latter cut
    to 3000 bytes: words of up to 3000 bytes that end one to three tiles further on, on tile limits, at a document's or the
    batch's end.  The exception kernels are k_tiles' own, the records they start from are k_ptiles'.  Twin."""
    ctx, orc = _pair(vocabs, oracle_mod, name)
    docs, word = H.later_tile_word_docs()
    _check(ctx, orc, docs[::2] if name == "RB" else docs, "ends")
    _check(ctx, orc, [d[:3000] for d in H.long_word_docs()] + [word(3000)], "long")


# ---- 6. documents ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", TAKEN)
def test_document_bookkeeping(forced, vocabs, oracle_mod, name):
    """More than 64 document starts in a tile -- the front end and the epilogue fetch offsets[dfirst + lane], 64 at a
    time: 65, 128 and 960 one-byte documents in a tile; runs of empty documents at the start of the batch, on and around
    a tile limit, inside the look-back, and at the end; a batch whose only document with bytes is the last; an all-empty
    batch (nothing is launched: hutk_debug_tile_kernel says 0 for it); the ragged packing of
    test_document_boundaries_inside_characters.  Twin."""
    ctx, orc = _pair(vocabs, oracle_mod, name)
    for tag, docs in _document_batches():
        _check(ctx, orc, docs, "%s %s" % (name, tag))
    _check(ctx, orc, [b""] * 100, "all empty")
    _check(ctx, orc, [b""], "one empty document")


# ---- 7. arbitrary bytes ----------------------------------------------------------------------------------------

def _arbitrary_docs():
    rng = random.Random(77)
    high = [bytes([b]) for b in range(0xF5, 0x100)] + [b"\xf4\x90\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xed\xa0\x80", b"\xe0\x9f\xbf",
                                                     b"\xf0\x8f\xbf\xbf", b"\xf0\x9f\x98", b"\xef\xbf\xbd", b"\xe2\x80\xa8"]
    docs = []
    for _ in range(3000):
        parts = [H.random_bytes_text(rng, rng.randint(0, 12)) if rng.random() < 0.7 else rng.choice(high)
                 for _ in range(rng.randint(0, 12))]
        docs.append(b"".join(parts))
    return docs


@pytest.mark.parametrize("name", ["RB", "VG"])
def test_arbitrary_bytes(forced, vocabs, oracle_mod, name):
    """3000 documents of random_bytes_text -- truncated, overlong and invalid UTF-8 -- with the bytes 0xF5 .. 0xFF, surrogates
    and sequences beyond U+10FFFF among them (the classifier's per-position decode keeps its window in the slot's symbol
    array meanwhile).  Twin."""
    ctx, orc = _pair(vocabs, oracle_mod, name)
    _check(ctx, orc, _arbitrary_docs(), "bytes")


def test_a_vocabulary_the_kernel_refuses(forced, vocabs, oracle_mod):
    """random_byte_vocab(3) with duplicate ids: ids do not rise with the symbols (rank_is_sym == 0), so ptiles_takes says no:
    hutk_debug_tile_kernel reports 0 with both switches set, and the ids are those of the oracle all the same."""
    ctx, orc = _pair(vocabs, oracle_mod, "RX")
    assert ctx.table_stats()["rank_is_sym"] == 0
    rng = random.Random(31)
    docs = [H.random_text(rng, max_words=40).encode("utf-8") for _ in range(1500)] + _arbitrary_docs()[:1500]
    assert ctx.tile_kernel(sum(map(len, docs))) == 0
    _check(ctx, orc, docs, "refused", want=0, twin=False)
    _check(ctx, orc, [_text(961)], "refused, two tiles", want=0, twin=False)


# ---- 8. NUL and over-long words --------------------------------------------------------------------------------

def test_nul_bytes(forced, vocabs, oracle_mod):
    """A 0x00 byte 0, 15, 16 and 959 bytes into the first, the second and the last tile, and as the last byte of the batch: the
    error word is HUTK_E_NUL_BYTE whichever lane's sixteen positions hold it, and error word and status are those of k_tiles
    on the same buffers.  (The ids of such a batch are not defined.)"""
    ctx, _orc = _pair(vocabs, oracle_mod, "VG")
    text = np.frombuffer(_text(3 * TILE + 200), dtype=np.uint8)
    offs = np.array([0, 100, 1000, 1000, len(text)], dtype=np.int64)
    places = [t * TILE + p for t in (0, 1, 3) for p in (0, 15, 16, 959) if t * TILE + p < len(text)] + [len(text) - 1]
    assert len(places) == 12
    for at in places:
        d = text.copy()
        d[at] = 0
        assert ctx.tile_kernel(len(d)) == 1
        b = _Batch(ctx, d, offs)
        _ids, _oo, st, err = b.run()
        assert err == E_NUL_BYTE, at
        with _env(HUTK_PTILES="0"):
            assert ctx.tile_kernel(len(d)) == 0
            _ids0, _oo0, st0, err0 = b.run()
        assert err0 == err and np.array_equal(st0, st), at
    _check(ctx, _orc, [text.tobytes()], "the context still encodes")


@pytest.mark.parametrize("seams", [True, False])
def test_over_long_words_cut_their_documents(forced, vocabs, oracle_mod, seams):
    """The documents of tests/test_gpu_cut.py: a word of more than MAX_WORD_BYTES = 262144 bytes ends its document.  k_cut works
    from cutpos / tile_lastreal and noreal_bits, which k_ptiles writes per tile.  With the seam map (a run of three-byte
    characters is thousands of short words) and without it (HUTK_NO_SEAM=1: one exception word).  Twin."""
    import test_gpu_cut as TC
    ctx, orc = _pair(vocabs, oracle_mod, "VG", **({} if seams else {"HUTK_NO_SEAM": "1"}))
    seam, _ = ctx.seam_map()
    assert _seams_on(ctx) == seams
    if seams:
        docs, want_st = TC.cut_docs(TC.quiet_char(orc, seam))
    else:
        docs, want_st = TC.NO_SEAM_DOCS, TC.NO_SEAM_STATUS
    from oracle import oracle as O
    data, offs = O.pack(docs)
    assert orc.encode_packed(data, offs, 8)[2].tolist() == want_st
    _check(ctx, orc, docs, "cut", want_rc=E_WORD_TOO_LARGE)


# ---- 9. seam switches on small CJK batches ---------------------------------------------------------------------

@pytest.mark.parametrize("switches", [{}, {"HUTK_NO_SEAM2": "1"}, {"HUTK_NO_SEAM": "1"}], ids=["seams", "no-seam2", "no-seam"])
@pytest.mark.parametrize("name", ["VC", "VG"])
def test_seams_on_small_cjk_batches(forced, vocabs, oracle_mod, name, switches):
    """synth.cjk_paragraphs and synth.cjk_text cut to 3, G + 1 and 2 G + 1 tiles: the seam map's two levels (k_ptiles asks the
    second, k_tiles does not), each switched off in turn; without seams every paragraph is one word of several hundred
    bytes.  Twin."""
    G = _grid()
    ctx, orc = _pair(vocabs, oracle_mod, name, **switches)
    assert _seams_on(ctx) == ("HUTK_NO_SEAM" not in switches)
    for gen in ("cjk_paragraphs", "cjk_text"):
        for n in (3, G + 1, 2 * G + 1):
            _check(ctx, orc, _cjk_tiles(gen, n), "%s %s %d tiles %s" % (name, gen, n, switches))


# ---- 10. the layers that cut text into pieces ------------------------------------------------------------------

def test_special_tokens_over_the_forced_kernel(forced, oracle_mod):
    """The inputs of test_scan_boundaries and test_stitch (tests/test_gpu_specials.py) against tests/specials_ref.py: the pieces
    between markers reach the tile kernel as a batch of many tiny and empty documents."""
    import test_gpu_specials as TS
    ctx, orc = TS._pair(oracle_mod, "VG")
    assert ctx.tile_kernel(1) == 1 and ctx.tile_kernel(40 * TILE) == 1
    docs, specials, n_in = TS.scan_boundaries_case()
    TS._check(ctx, orc, docs, dict(TS.VG_MARKERS, **specials), "scan boundaries, forced", min_matches=n_in + 1)
    for docs, tag, least in TS.stitch_cases():
        TS._check(ctx, orc, docs, TS.VG_MARKERS, tag + ", forced", min_matches=least)
    ctx.set_special_tokens([])


def test_byte_fallback_over_the_forced_kernel(forced, tmp_path, oracle_mod):
    """The byte vocabulary with holes of tests/test_gpu_fallback.py against tests/fallback_ref.py."""
    import spans_ref as S
    import test_gpu_fallback as TF
    ctx, orc, table, d, o = TF.holes_case(tmp_path, oracle_mod)
    assert ctx.tile_kernel(int(o[-1])) == 1
    TF._check_encode(ctx, S.TokenText(orc), d, o, True, table, "byte vocab with holes, forced")
    ctx.close()


def test_token_spans_of_a_forced_encode(forced, vocabs, oracle_mod):
    """The ragged batch of item 6 encoded by the forced kernel, then the span of every id against tests/spans_ref.py."""
    import spans_ref as S
    from oracle import oracle as O
    ctx, orc = _pair(vocabs, oracle_mod, "VG")
    d, o = O.pack(H.ragged_docs())
    assert ctx.tile_kernel(len(d)) == 1
    ids, oo, st, err = _Batch(ctx, d, o).run()
    assert err == 0 and not st.any()
    tt = S.TokenText(orc)
    for unit, code in (("byte", 0), ("char", 1)):
        want, wst = S.batch(tt, d, o, ids, oo, True, unit, np.int64)
        assert not wst.any()
        got, gst, rc = ctx.token_spans_packed(d, o, ids, oo, unit=code, out_width=8)
        assert rc == 0 and not gst.any()
        assert np.array_equal(got, want), unit


# ---- 11. auto mode on small batches ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["VG", "VC"])
def test_auto_mode_on_small_batches(auto, vocabs, oracle_mod, name):
    """Both kernels enqueued (hutk_debug_tile_kernel says 2), the choice made on the device from k_pre's sample: the batches of
    items 1, 2, 6 and 9.  Which of the two ran is not observable and not asserted: whichever it was, exactly one of them
    must have written the workspace."""
    G = _grid()
    ctx, orc = _pair(vocabs, oracle_mod, name)
    batches = _partial_window_batches() + _document_batches()
    batches += [("C3 %d tiles" % n, _c3_tiles(n)) for n in (G - 1, G, G + 1, 2 * G - 1, 2 * G + 1)]
    batches += [("%s %d tiles" % (gen, n), _cjk_tiles(gen, n)) for gen in ("cjk_paragraphs", "cjk_text") for n in (3, G + 1, 2 * G + 1)]
    for tag, docs in batches:
        _check(ctx, orc, docs, "auto %s %s" % (name, tag), want=2, twin=False)


def test_auto_mode_at_the_density_threshold(auto, vocabs, oracle_mod):
    """k_pre looks at the 16 bytes 480 .. 495 of every tile (of a batch of up to 256 tiles) and counts those >= 0xE0; the batch is
    dense when count * SELECT_DENSE_DIV * SELECT_BLOCK_STRIDE (8 * 8) >= n_tiles * SELECT_SAMPLE (16).  Sixteen tiles of
    ASCII text with four three-byte characters in the sampled places sit exactly on the threshold, with three of them one
    below it; and a batch under 496 bytes has nothing to sample.  Every one equals the oracle."""
    ctx, orc = _pair(vocabs, oracle_mod, "VG")
    rng = random.Random(16)
    n_tiles = 16
    base = bytearray()
    while len(base) < n_tiles * TILE - 100:
        base += H.random_text(rng, max_words=40, exotic=0.0).encode("ascii", "ignore") + b" "
    del base[n_tiles * TILE - 100:]
    assert max(base) < 0x80
    han = "漢".encode()
    places = [3 * TILE + 480, 3 * TILE + 493, 7 * TILE + 485, 12 * TILE + 480]
    at, below = bytearray(base), bytearray(base)
    for k, p in enumerate(places):
        at[p:p + 3] = han
        if k:
            below[p:p + 3] = han

    def sampled(buf):
        return sum(1 for t in range(n_tiles) for b in buf[t * TILE + 480:t * TILE + 496] if b >= 0xE0)
    assert sampled(at) * 8 * 8 == n_tiles * 16 and sampled(below) == sampled(at) - 1
    for tag, buf in (("on the threshold", at), ("one below", below), ("none", base)):
        _check(ctx, orc, [bytes(buf[:5000]), bytes(buf[5000:])], "auto " + tag, want=2, twin=False)
    for docs in ([han * 165], [han * 160, b" and text"], [_text(495)], [_text(496)], [han * 166]):
        assert 480 <= sum(map(len, docs)) <= 498
        _check(ctx, orc, docs, "auto %d bytes" % sum(map(len, docs)), want=2, twin=False)


def test_auto_mode_sequences_on_one_context(auto, vocabs, oracle_mod):
    """On ONE context and one stream, nothing made anew in between: dense, Latin, empty (n_tiles == 0 returns before k_pre);
    then dense, a batch that ends in a NUL error, Latin, dense.  k_pre's count (CTR_SELECT_HI) is cleared by the tail of the
    batch before: a stale count would show as both kernels, or neither, writing the workspace.  Every step equals the
    oracle; the NUL batch raises HUTK_E_NUL_BYTE."""
    from oracle import oracle as O
    ctx, orc = _pair(vocabs, oracle_mod, "VG")
    stream = _stream()
    dense, latin = _cjk_tiles("cjk_paragraphs", 24), _c3_tiles(24)
    small_dense, small_latin = _cjk_tiles("cjk_text", 3), [_text(2000)]  # (three tiles: the small tail clears the count)
    nul = np.frombuffer(b"".join(dense), dtype=np.uint8).copy()
    nul[len(nul) // 2] = 0

    def step(docs, tag):
        data, offs = O.pack(docs)
        assert ctx.tile_kernel(len(data)) == (2 if len(data) else 0)
        want = orc.encode_packed(data, offs, 4)
        ids, oo, st, err = _Batch(ctx, data, offs).run(stream)
        assert err == 0, tag
        assert np.array_equal(oo, want[1]) and np.array_equal(ids, want[0]) and np.array_equal(st, want[2]), tag

    def nul_step(tag):
        offs = np.array([0, len(nul)], dtype=np.int64)
        assert ctx.tile_kernel(len(nul)) == 2
        assert _Batch(ctx, nul, offs).run(stream)[3] == E_NUL_BYTE, tag
    for a, b, tag in ((dense, latin, "24 tiles"), (small_dense, small_latin, "3 tiles")):
        step(a, "dense, " + tag)
        step(b, "latin behind dense, " + tag)
        step([b"", b""], "empty, " + tag)
        step(a, "dense behind empty, " + tag)
        nul_step("nul, " + tag)
        step(b, "latin behind nul, " + tag)
        step(a, "dense behind latin, " + tag)
        step(small_latin, "small latin, " + tag)
        step(a, "dense at the end, " + tag)
