"""The GPU trainer's internal paths (hutk_train.hip), each forced or reached on purpose and shown to be taken by
Trainer.debug_counters(): pauses, growth and shrinking of the pair table, k_select at its 1024-block cap, long words
that become short and long words whose pair lies past symbol 64, counts above 2^32, symbol ids above 65535, deferred
inserts and word-table rehashes between add() calls.  Every answer is compared exactly with tests/train_ref.py or
tools/train_vocab.cpp.  The schedule knobs HUTK_TRAIN_SYNC_EVERY and HUTK_TRAIN_PAIR_CAP_LOG2 are read by every run()."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import helpers
import train_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("HUTK_TRAIN_SYNC_EVERY", "HUTK_TRAIN_PAIR_CAP_LOG2")


def _pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


def _knobs(monkeypatch, sync=None, cap_log2=None):
    for name, v in zip(KNOBS, (sync, cap_log2)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _gpu(batches, n_merges):
    """batches: list of (data, offsets) -> (pairs [(a, b)], counts [int], debug counters)."""
    import hutoken_amd as H
    with H.Trainer() as t:
        for data, offs in batches:
            t.add_packed(data, offs)
        p, c = t.run(n_merges)
        return [tuple(x) for x in p.tolist()], c.tolist(), t.debug_counters()


# ---- schedule invariance ----------------------------------------------------------------------------------------

def _schedule_corpus():
    rng = random.Random(0x5C4D)
    docs = [helpers.random_text(rng, max_words=20, exotic=0.5).encode("utf-8") for _ in range(250)]
    docs += [helpers.random_bytes_text(rng, rng.randint(0, 50)) for _ in range(80)]
    for _ in range(200):  # tie-heavy: the same few pairs in equal numbers
        docs.append(b" ".join(bytes([97 + rng.randrange(5), 97 + rng.randrange(5)]) for _ in range(rng.randint(1, 12))))
    return docs


def test_schedule_invariance(monkeypatch):
    docs = _schedule_corpus()
    want = train_ref.train(docs, 10**6)
    assert 3000 < len(want[0]) < 10**6 and want[1][-1] == 1  # down to count 1
    batch = [_pack(docs)]
    seen = {}
    for sync in (1, 3, None, 100000):
        for cap in (8, None, 21):
            _knobs(monkeypatch, sync, cap)
            p, c, dc = _gpu(batch, 10**6)
            assert (p, c) == want, (sync, cap)
            seen[(sync, cap)] = dc
    assert any(dc["pauses"] > 0 for dc in seen.values())
    assert any(dc["pair_shrinks"] > 0 for dc in seen.values())
    assert any(dc["pair_grows"] > 0 for dc in seen.values())
    print({k: (dc["pauses"], dc["pair_grows"], dc["pair_shrinks"], dc["host_syncs"], dc["pair_cap_max"])
           for k, dc in seen.items()})
    for cap in (8, None, 21):  # no synchronisation there but the pauses and the end
        assert seen[(100000, cap)]["host_syncs"] == seen[(100000, cap)]["pauses"] + 1
    assert seen[(1, None)]["host_syncs"] >= len(want[0])
    for sync in (1, 3, None, 100000):
        assert seen[(sync, 21)]["select_blocks_max"] == 1024 and seen[(sync, 21)]["pair_cap_max"] >= 1 << 21
        assert seen[(sync, None)]["select_blocks_max"] < 1024
    # the largest floor three times (eight and more grid-stride trips per thread): identical, ties included
    _knobs(monkeypatch, None, 22)
    for _ in range(3):
        p, c, dc = _gpu(batch, 10**6)
        assert (p, c) == want
        assert dc["select_blocks_max"] == 1024 and dc["pair_cap_max"] >= 1 << 22


# ---- counts past 2^32 -------------------------------------------------------------------------------------------

def test_counts_past_2_32(monkeypatch):
    _knobs(monkeypatch)
    n_docs, doc = 1 << 20, 1024  # 1 GiB: half b"a" * 1024, half b"b" * 1024; every document is one word
    data = np.empty(n_docs * doc, dtype=np.uint8)
    data[:n_docs * doc // 2] = ord("a")
    data[n_docs * doc // 2:] = ord("b")
    offs = np.arange(0, n_docs * doc + 1, doc, dtype=np.int64)
    adds = 9
    p, c, dc = _gpu([(data, offs)] * adds, 100)
    del data
    n = adds * n_docs // 2
    want = train_ref.train_words({b"a" * doc: n, b"b" * doc: n}, 100)
    assert (p, c) == want
    assert c[0] == c[1] == n * (doc - 1) > 2**32
    assert p[:2] == [(97, 97), (98, 98)]  # the tie goes to the smaller key
    assert dc["deferred_words"] > 0 and dc["insert_rounds_max"] >= 1


# ---- long-word geometry -----------------------------------------------------------------------------------------

def _fill(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


def _long_word_corpus():
    docs = [b"xz" + b" xz" * 99] * 100  # (x, z) wins the first merge: 10,000
    units = [b"cd", b"cde", b"cdef", b"gh", b"ghk", b"mnmnp"]
    for i, n in enumerate((63, 64, 65, 66, 127, 128, 129, 130, 1000)):
        for u in units[i % 3::3]:  # they shrink across the 64-symbol line as training goes on
            docs += [_fill(u, n)] * (2 + i % 3)
    # the only (x, z) of a long word straddles 63|64 or 127|128, or lies past symbol 64
    for j, n in ((62, 130), (63, 130), (64, 130), (100, 200), (126, 200), (127, 200), (128, 200), (500, 1000),
                 (935, 1000)):
        w = _fill(b"gh", j) + b"xz" + _fill(b"cd", n - j - 2)
        assert len(w) == n and w.count(b"xz") == 1
        docs += [w] * 2
    return docs


@pytest.mark.parametrize("sync", [1, None])
def test_long_word_geometry(monkeypatch, sync):
    docs = _long_word_corpus()
    want = train_ref.train(docs, 10**6)
    assert want[0][0] == (ord("x"), ord("z"))
    _knobs(monkeypatch, sync)
    p, c, dc = _gpu([_pack(docs)], 10**6)
    assert (p, c) == want
    assert dc["long_to_short"] > 0


# ---- symbol ids >= 65536 ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trainer_exe(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_vocab
    return make_vocab.build_trainer(str(tmp_path_factory.mktemp("train_vocab")))


def _tokens(pairs):
    toks = [bytes([b]) for b in range(256)]
    for a, b in pairs:
        toks.append(toks[a] + toks[b])
    return toks


def test_symbols_past_16_bits(monkeypatch, tmp_path, trainer_exe, oracle_mod):
    import hutoken_amd as H
    from hutoken_amd import synth
    from hutoken_amd import vocab_files as vf
    _knobs(monkeypatch)
    seed, n_docs, n_merges = 0x564F4347, 125000, 70000
    d, o = synth.corpus("C3", n_docs, seed=seed)
    p, c, _ = _gpu([(d, o)], n_merges)
    assert len(p) >= 66000
    assert max(max(ab) for ab in p) >= 65536
    pf = str(tmp_path / "pairs.txt")
    subprocess.run([trainer_exe, "3", str(seed), str(n_docs), str(n_merges), str(tmp_path / "out.txt"), "bytes", pf],
                   check=True, capture_output=True)
    cpp = [tuple(bytes.fromhex(x) for x in ln.split()) for ln in open(pf)]
    toks = _tokens(p)
    assert [(toks[a], toks[b]) for a, b in p] == cpp
    assert c == sorted(c, reverse=True) and c[-1] >= 1
    # the same with no synchronisation but the pauses: the device-side check alone keeps the pair table from filling
    _knobs(monkeypatch, 100000)
    p2, c2, dc = _gpu([(d, o)], n_merges)
    print(dc)
    assert (p2, c2) == (p, c)
    assert dc["pauses"] > 0 and dc["host_syncs"] == dc["pauses"] + 1 and dc["pair_grows"] > 0
    _knobs(monkeypatch)

    paths = vf.write_gpt2_files(str(tmp_path), "big", p)
    hd, ho = synth.corpus("C3", 3000, seed=0x686F6C64)  # held out
    orc = oracle_mod.Oracle(paths["vocab_file"], paths["special_file"], None, True)
    want, want_o, _ = orc.encode_packed(hd, ho, 4)
    assert int(want.max()) >= 65536
    raw = hd.tobytes()
    texts = [raw[ho[i]:ho[i + 1]].decode("utf-8") for i in range(len(ho) - 1)]
    for merges in (None, paths["merges_file"]):
        kw = {} if merges is None else {"merges_file_path": merges}
        H.initialize(paths["vocab_file"], paths["special_file"], is_byte_encoder=True, **kw)
        ids, oo, _ = H.encode_packed(hd, ho)
        assert np.array_equal(oo, want_o) and np.array_equal(ids, want), merges
        per_doc = [ids[oo[i]:oo[i + 1]].tolist() for i in range(len(oo) - 1)]
        assert H.batch_decode(per_doc) == texts


# ---- batches and the word table ---------------------------------------------------------------------------------

def test_batches_and_word_table(monkeypatch):
    _knobs(monkeypatch)
    rng = random.Random(0xBA7C)
    pool = [helpers.random_text(rng, max_words=20, exotic=0.4).encode("utf-8") for _ in range(3000)]
    pool += [helpers.random_bytes_text(rng, rng.randint(1, 30)) for _ in range(200)] + [b""] * 50
    sizes = [10, 0, 100, 1000, 10000, 100000]
    order = [[rng.randrange(len(pool)) for _ in range(k)] for k in sizes]
    batches = [_pack([pool[i] for i in idx]) for idx in order]
    batches.insert(1, _pack([b"", b"", b""]))
    # a slice of a larger packed buffer: offsets[0] > 0
    outer = [pool[rng.randrange(len(pool))] for _ in range(500)]
    od, oo = _pack(outer)
    batches.append((od, oo[100:401]))
    everything = [pool[i] for idx in order for i in idx] + outer[100:400]

    p, c, dc = _gpu(batches, 4000)
    p1, c1, _ = _gpu([_pack(everything)], 4000)
    assert (p, c) == (p1, c1)
    assert dc["word_rehashes"] >= 2
    mult = {}
    for d in everything:
        mult[d] = mult.get(d, 0) + 1
    counts = {}
    for d, m in mult.items():
        for w, k in train_ref.word_counts([d]).items():
            counts[w] = counts.get(w, 0) + k * m
    assert (p, c) == train_ref.train_words(counts, 4000)


# ---- n_merges bounds --------------------------------------------------------------------------------------------

def test_n_merges_bounds(monkeypatch):
    import hutoken_amd as H
    _knobs(monkeypatch)
    docs = [b"the cat sat on the mat", b"hello world"]
    want = train_ref.train(docs, 10_000)
    with H.Trainer() as t:
        t.add_packed(*_pack(docs))
        for bad in (2**31, 2**32 + 5):
            with pytest.raises(ValueError):
                t.run(bad)
        p, c = t.run(10**9)  # the trainer has not run yet: the bad calls allocated and ran nothing
    assert ([tuple(x) for x in p.tolist()], c.tolist()) == want
    p2, c2, _ = _gpu([_pack(docs)], 10_000)
    assert (p2, c2) == want and 0 < len(p2) < 10_000
