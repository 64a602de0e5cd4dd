"""GPU training in chars mode (hutk_train.hip symbolisation, Trainer(mode="chars"), train(mode="chars")) against
tests/train_ref_chars.py, tools/train_vocab.cpp ... chars and the committed VL files (data/vl32000_*)."""
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import helpers
import train_ref
import train_ref_chars as R

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


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    _knobs(monkeypatch)


def _gpu(batches, n_merges):
    """batches: list of (data, offsets) -> (alphabet, pairs [(a, b)], counts [int], debug counters, stats)."""
    import hutoken_amd as H
    with H.Trainer(mode="chars") as t:
        for data, offs in batches:
            t.add_packed(data, offs)
        alphabet = t.alphabet()
        assert t.alphabet() == alphabet  # the same answer every time
        p, c = t.run(n_merges)
        return alphabet, [tuple(x) for x in p.tolist()], c.tolist(), t.debug_counters(), t.stats()


def _check(docs, n_merges, batches=None):
    want = R.train(docs, n_merges)
    alphabet, p, c, dc, st = _gpu(batches or [_pack(docs)], n_merges)
    assert alphabet == want[0]
    assert p == want[1]
    assert c == want[2]
    assert dc["dropped_words"] == want[3]
    return want, dc, st


def test_random_corpora():
    rng = random.Random(0xC4A2)
    for trial in range(4):
        docs = R.edge_docs(rng)[:rng.randint(50, 400)]
        docs += [helpers.random_text(rng, max_words=30, exotic=0.6).encode("utf-8") for _ in range(100)]
        want, dc, _ = _check(docs, rng.choice([1, 50, 400, 3000]))
        assert dc["dropped_words"] > 0


def test_symbol_count_and_drop_counter():
    docs = [b"ab \xe2\x96\x81cd", b"x\x01yz", b"\xe2 x \x7fq", b"\xf0ab"]
    alphabet, words, n_drop = R.symbolise(train_ref.word_counts(docs))
    got = _gpu([_pack(docs)], 5)
    assert got[0] == alphabet
    assert got[3]["dropped_words"] == n_drop == 2
    assert got[4]["symbols"] == sum(len(w) for w in words)  # characters of the kept unique words


def test_runs_and_ties():
    docs = [b"a" * k for k in range(1, 10)] + [b"ab" * k for k in range(1, 12)] + [b"aab" * 7 + b" " + b"a" * 17]
    docs += [("é" * k).encode("utf-8") for k in range(1, 9)] + [("éa" * 5 + " " + "漢" * 9).encode("utf-8")]
    _check(docs, 60)
    words = ["%s%s" % (x, y) for x in "aé漢😂" for y in "bß字🙂"]
    _check([" ".join(words).encode("utf-8")] * 3 + ["".join(c + " " for c in "xyzñ").encode("utf-8")], 200)


def _fill(unit, n_chars):
    return ((unit * (n_chars // len(unit) + 1))[:n_chars]).encode("utf-8")


def test_long_words(monkeypatch):
    rng = random.Random(0x10A6)
    big = "".join(rng.choice(["a", "b", "é", "ß", "漢", "字", "😂"]) for _ in range(140_000)).encode("utf-8")
    big = big[:150_000] + b"\xe2" + big[150_000:300_000]  # one 300 KB word with a stray lead byte inside
    assert len(big) == 300_001
    _check([big], 12)
    docs = [("ΧΨ" + " ΧΨ" * 99).encode("utf-8")] * 100  # (Χ, Ψ) wins the first merge
    # the only (Χ, Ψ) of a long word sits at characters 62..63, 63..64, 64..65, 126..127, 127..128 or past 64
    for j, n in ((62, 130), (63, 130), (64, 130), (126, 200), (127, 200), (128, 200), (500, 1000)):
        w = _fill("漢字", j) + "ΧΨ".encode("utf-8") + _fill("éß", n - j - 2)
        assert len(w.decode("utf-8")) == n
        docs += [w] * 2
    # CJK paragraphs: one word each, 100-400 characters
    from hutoken_amd import synth
    d, o = synth.cjk_text(60, seed=0x4C57)
    raw = d.tobytes()
    docs += [p for i in range(len(o) - 1) for p in raw[o[i]:o[i + 1]].split(b"\n")]
    want = R.train(docs, 400)
    assert want[1][0] == (want[0].index("Χ".encode("utf-8")), want[0].index("Ψ".encode("utf-8")))
    for sync in (1, None):
        _knobs(monkeypatch, sync)
        alphabet, p, c, dc, _ = _gpu([_pack(docs)], 400)
        assert (alphabet, p, c) == tuple(want[:3]), sync
        assert dc["long_to_short"] > 0


def _wide_pair_corpus():
    """About 300,000 unique two-character words over 600 CJK characters: more distinct pairs at the start than bytes
    mode's initial pair table bound (4 x 65,536 slots) allows."""
    rng = random.Random(0x3A1F)
    chars = [chr(0x4E00 + i) for i in range(600)]
    pairs = [(x, y) for x in chars for y in chars]
    rng.shuffle(pairs)
    words = [" " + x + y for x, y in pairs[:300_000]]
    words += [" " + x + y for x, y in pairs[:2000]] * 3  # a few counts above 1
    return [" ".join(words[i:i + 1000]).encode("utf-8") for i in range(0, len(words), 1000)]


def test_initial_pairs_past_the_byte_bound():
    docs = _wide_pair_corpus()
    want, _, st = _check(docs, 40)
    assert st["pairs_at_start"] > 4 * 65536
    assert len(want[0]) == 601 and len(want[1]) == 40


def test_charset_regrowth(monkeypatch):
    rng = random.Random(0xC5E7)
    docs = R.edge_docs(rng) + [helpers.random_text(rng, max_words=20, exotic=0.7).encode("utf-8") for _ in range(300)]
    monkeypatch.setenv("HUTK_TRAIN_CHARSET_CAP_LOG2", "4")
    want, dc, _ = _check(docs, 500)
    assert len(want[0]) > 64 and dc["charset_grows"] >= 2
    monkeypatch.delenv("HUTK_TRAIN_CHARSET_CAP_LOG2")
    _, dc, _ = _check(docs, 500)
    assert dc["charset_grows"] == 0


def test_all_dropped(tmp_path):
    import hutoken_amd as H
    docs = [b"\x01\x02", b"\t", b"\x7f", b"\x1f\x1e"]
    alphabet, p, c, dc, st = _gpu([_pack(docs)], 10)
    assert alphabet == [] and p == [] and c == [] and st["symbols"] == 0
    assert dc["dropped_words"] == len(train_ref.word_counts(docs)) > 0
    out = H.train([d.decode("ascii") for d in docs], 259, str(tmp_path), "empty", mode="chars")
    assert out["alphabet_size"] == 0 and out["n_merges"] == 0
    assert len(open(out["vocab_file"]).read().splitlines()) == 259
    assert open(out["merges_file"], "rb").read() == b"#version: 0.2\n"


def test_batches():
    rng = random.Random(0xBA7D)
    pool = R.edge_docs(rng) + [helpers.random_text(rng, max_words=20, exotic=0.5).encode("utf-8") for _ in range(800)]
    sizes = [10, 0, 100, 1000, 3000]
    batches = [_pack([pool[rng.randrange(len(pool))] for _ in range(k)]) for k in sizes]
    everything = [bytes(d[o[i]:o[i + 1]]) for d, o in batches for i in range(len(o) - 1)]
    _, dc, _ = _check(everything, 2000, batches=batches)
    assert dc["word_rehashes"] >= 1


def test_schedule_knobs(monkeypatch):
    rng = random.Random(0x5C4E)
    docs = R.edge_docs(rng) + [helpers.random_text(rng, max_words=20, exotic=0.6).encode("utf-8") for _ in range(300)]
    want = R.train(docs, 10**6)
    assert want[2][-1] == 1  # down to count 1
    seen = {}
    for sync, cap in ((1, None), (1, 8), (None, 8), (100000, 8)):
        _knobs(monkeypatch, sync, cap)
        alphabet, p, c, dc, _ = _gpu([_pack(docs)], 10**6)
        assert (alphabet, p, c) == tuple(want[:3]), (sync, cap)
        seen[(sync, cap)] = dc
    print({k: (dc["pauses"], dc["pair_grows"], dc["pair_shrinks"], dc["host_syncs"]) for k, dc in seen.items()})
    assert seen[(1, None)]["host_syncs"] >= len(want[1])
    assert any(dc["pauses"] > 0 for dc in seen.values())
    assert any(dc["pair_grows"] > 0 for dc in seen.values())
    assert any(dc["pair_shrinks"] > 0 for dc in seen.values())
    assert seen[(100000, 8)]["host_syncs"] == seen[(100000, 8)]["pauses"] + 1


def test_alphabet_contract():
    import hutoken_amd as H
    docs = [b"hello w\xc3\xb6rld", b"\xe6\xbc\xa2\xe5\xad\x97 ok"]
    with H.Trainer(mode="chars") as t:
        t.add_packed(*_pack(docs))
        a = t.alphabet()
        assert a == R.symbolise(train_ref.word_counts(docs))[0]
        with pytest.raises(TypeError):
            t.add_packed(*_pack([b"more"]))
        p, _ = t.run(100)
        assert t.alphabet() == a  # still readable after run
    assert max(max(x) for x in p.tolist()) >= len(a)  # merge symbols start at A
    with H.Trainer() as t:
        t.add(["bytes mode"])
        assert t.alphabet() == [bytes([b]) for b in range(256)]
        with pytest.raises(TypeError):
            t.add(["more"])
        p, _ = t.run(5)
    assert [tuple(x) for x in p.tolist()] == train_ref.train([b"bytes mode"], 5)[0]


def test_train_vocab_too_small(tmp_path):
    import hutoken_amd as H
    texts = ["héllo wörld", "日本語 text"]
    A = len(R.symbolise(train_ref.word_counts([t.encode("utf-8") for t in texts]))[0])
    with pytest.raises(RuntimeError, match=r"A = %d\b" % A):
        H.train(texts, 259 + A - 1, str(tmp_path), "small", mode="chars")
    assert os.listdir(tmp_path) == []
    out = H.train(texts, 259 + A, str(tmp_path), "fits", mode="chars")
    assert out["alphabet_size"] == A and out["n_merges"] == 0


def _gunzip(name):
    with gzip.open(os.path.join(ROOT, "data", name), "rb") as f:
        return f.read()


def test_vl_golden(tmp_path):
    import hutoken_amd as H
    from hutoken_amd import synth
    d, o = synth.corpus("C5", 60000, seed=0x564F434C)
    raw = d.tobytes()
    texts = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    out = H.train([texts[:25000], texts[25000:]], 32000, str(tmp_path), "vl", mode="chars")
    assert out["alphabet_size"] == 57 and out["n_merges"] == 31684
    assert open(out["vocab_file"], "rb").read() == _gunzip("vl32000_vocab.txt.gz")
    assert open(out["special_file"], "rb").read() == open(os.path.join(ROOT, "data", "vl32000_special.txt"), "rb").read()


@pytest.fixture(scope="module")
def trainer_exe(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_vocab
    return make_vocab.build_trainer(str(tmp_path_factory.mktemp("train_vocab")))


def test_cjk_subset_vs_cpp(tmp_path, trainer_exe):
    from hutoken_amd import synth
    d, o = synth.cjk_text(600, seed=0x56435452)
    raw = d.tobytes()
    pars = [p for i in range(len(o) - 1) for p in raw[o[i]:o[i + 1]].split(b"\n")][:1500]
    assert len(pars) == 1500
    path = tmp_path / "cjk.txt"
    path.write_bytes(b"".join(p + b"\n" for p in pars))
    out, pf = str(tmp_path / "out.txt"), str(tmp_path / "pairs.txt")
    subprocess.run([trainer_exe, "0", str(path), "0", "2000", out, "chars", pf], check=True, capture_output=True)
    base = [bytes.fromhex(x) for x in open(out).read().split("--\n")[0].split()]
    cpp = [tuple(bytes.fromhex(x) for x in ln.split()) for ln in open(pf)]
    alphabet, p, _, _, _ = _gpu([_pack(pars)], 2000)
    assert alphabet == base and len(p) == 2000
    toks = R.tokens(alphabet, p)
    assert [(toks[a], toks[b]) for a, b in p] == cpp


def test_round_trip(tmp_path, oracle_mod):
    import hutoken_amd as H
    from hutoken_amd import synth
    d, o = synth.corpus("C5", 4000, seed=0x52545243)
    raw = d.tobytes()
    texts = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    out = H.train([texts[:1500], texts[1500:3000]], 3000, str(tmp_path), "rt", mode="chars")
    held = texts[3000:3300]
    orc = oracle_mod.Oracle(out["vocab_file"], out["special_file"], "▁", False)
    want = [orc.encode(t) for t in held]
    H.initialize(out["vocab_file"], out["special_file"], prefix="▁", is_byte_encoder=False)
    ids = H.batch_encode(held)
    assert ids == want
    assert H.batch_decode(ids) == [orc.decode(x) for x in want]
    orc_m = oracle_mod.Oracle(out["vocab_file"], out["special_file"], "▁", False, merges_path=out["merges_file"])
    assert orc_m.has_merges
    want_m = [orc_m.encode(t) for t in held]
    H.initialize(out["vocab_file"], out["special_file"], prefix="▁", is_byte_encoder=False,
                 merges_file_path=out["merges_file"])
    ids_m = H.batch_encode(held)
    assert ids_m == want_m
    # the id-keyed merge path gives -1 for a character the vocabulary lacks (as the oracle does), which no decoder
    # accepts: the documents without one are decoded
    whole = [x for x in ids_m if min(x, default=0) >= 0]
    assert 0 < len(whole) < len(ids_m)
    assert H.batch_decode(whole) == [orc_m.decode(x) for x in whole]
