"""GPU BPE training (hutk_trainer_*, hutoken_amd.Trainer / train / bpe_train) against tests/train_ref.py and the
committed vocabularies trained by tools/train_vocab.cpp (data/vg50257_*, data/vc12257_vocab.txt.gz)."""
import gzip
import os
import random

import numpy as np
import pytest

import helpers
import train_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


def _gpu(docs, n_merges, batches=1):
    import hutoken_amd as H
    with H.Trainer() as t:
        cut = np.linspace(0, len(docs), batches + 1).astype(int)
        for i in range(batches):
            t.add_packed(*_pack(docs[cut[i]:cut[i + 1]]))
        p, c = t.run(n_merges)
        return [tuple(x) for x in p.tolist()], c.tolist(), t.stats()


def _check(docs, n_merges):
    p, c, _ = _gpu(docs, n_merges)
    rp, rc = train_ref.train(docs, n_merges)
    assert p == rp
    assert c == rc
    return p


def test_random_corpora():
    rng = random.Random(0x7472)
    for trial in range(6):
        docs = [helpers.random_text(rng, max_words=30, exotic=0.5).encode("utf-8") for _ in range(rng.randint(1, 300))]
        docs += [helpers.random_bytes_text(rng, rng.randint(0, 60)) for _ in range(rng.randint(0, 40))]
        _check(docs, rng.choice([1, 50, 400, 3000]))


def test_runs_and_alternations():
    docs = [b"a" * k for k in range(1, 10)] + [b"ab" * k for k in range(1, 12)] + [b"aab" * 7 + b" " + b"a" * 17]
    _check(docs, 40)
    _check([b"a" * 9], 10)


def test_long_words():
    rng = random.Random(5)
    big = bytes(rng.choice(b"abcde") for _ in range(300_000))  # one 300 KB word
    mid = b"xy" * 40_000  # 80 KB
    alt = bytes(rng.choice(b"qrs") for _ in range(70_000))
    _check([big], 12)
    _check([mid, alt, b"hello " * 50], 30)


def test_high_bytes_and_invalid_utf8():
    rng = random.Random(9)
    docs = [bytes(rng.randint(0x80, 0xFF) for _ in range(rng.randint(1, 40))) for _ in range(200)]
    docs += [helpers.random_bytes_text(rng, 80) for _ in range(200)]
    _check(docs, 500)


def test_nothing_to_merge():
    for docs in ([b"", b"", b""], [b"a", b"b", b" ", b"\n"], []):
        p, c, st = _gpu(docs, 10)
        assert p == [] and c == []
    assert train_ref.train([b"a", b"b"], 10) == ([], [])


def test_ties():
    words = [bytes([97 + i, 97 + j]) for i in range(8) for j in range(8)]
    docs = [b" ".join(words)] * 3 + [b"".join(bytes([x]) + b" " for x in range(33, 127))]
    _check(docs, 200)


def test_more_merges_than_corpus_allows():
    docs = [b"the cat sat on the mat", b"hello world"]
    p = _check(docs, 10_000)
    assert 0 < len(p) < 10_000


def test_batching_and_doubling():
    rng = random.Random(77)
    docs = [helpers.random_text(rng, max_words=40).encode("utf-8") for _ in range(500)]
    p1, c1, _ = _gpu(docs, 800, batches=1)
    p7, c7, st = _gpu(docs, 800, batches=7)
    assert (p1, c1) == (p7, c7)
    assert st["docs"] == 500
    p2, c2, _ = _gpu(docs + docs, 800, batches=3)
    assert p2 == p1 and c2 == [2 * x for x in c1]
    pa, ca, _ = _gpu(docs, 800)
    assert (pa, ca) == (p1, c1)  # two runs, same output


def test_nul_byte_and_recovery():
    import hutoken_amd as H
    docs = [b"hello world", b"some more text here", b"again hello"]
    with H.Trainer() as t:
        t.add_packed(*_pack(docs[:1]))
        with pytest.raises(ValueError):
            t.add_packed(*_pack([b"bad\x00doc", b"never counted"]))
        t.add_packed(*_pack(docs[1:]))
        p, c = t.run(30)
        with pytest.raises(TypeError):
            t.run(30)  # run once per trainer
    rp, rc = train_ref.train(docs, 30)
    assert [tuple(x) for x in p.tolist()] == rp and c.tolist() == rc


def _gunzip(name):
    with gzip.open(os.path.join(ROOT, "data", name), "rb") as f:
        return f.read()


def test_vc_golden(tmp_path):
    import hutoken_amd as H
    from hutoken_amd import synth
    d, o = synth.cjk_text(8000, seed=0x56435452)
    raw = d.tobytes()
    texts = [par.decode("utf-8") for i in range(len(o) - 1) for par in raw[o[i]:o[i + 1]].split(b"\n")]
    assert len(texts) == 20072
    out = H.train(texts, 12257, str(tmp_path), "vc")
    assert out["n_merges"] == 12000
    assert open(out["vocab_file"], "rb").read() == _gunzip("vc12257_vocab.txt.gz")


def test_vg_golden(tmp_path):
    import hutoken_amd as H
    from hutoken_amd import synth
    d, o = synth.corpus("C3", 125000, seed=0x564f4347)
    with H.Trainer() as t:
        t.add_packed(d, o)
        pairs, _ = t.run(50000)
    from hutoken_amd import vocab_files as vf
    paths = vf.write_gpt2_files(str(tmp_path), "vg", pairs.tolist())
    assert open(paths["vocab_file"], "rb").read() == _gunzip("vg50257_vocab.txt.gz")
    assert open(paths["merges_file"], "rb").read() == _gunzip("vg50257_merges.txt.gz")


def test_round_trip(tmp_path, oracle_mod):
    import hutoken_amd as H
    from hutoken_amd import synth
    d, o = synth.corpus("C3", 3000, seed=0x1234)
    raw = d.tobytes()
    texts = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
    out = H.train([texts[:1000], texts[1000:2000]], 2000, str(tmp_path), "rt")
    H.initialize(out["vocab_file"], out["special_file"], is_byte_encoder=True)
    held = texts[2000:2200]
    ids = H.batch_encode(held)
    assert H.batch_decode(ids) == held
    orc = oracle_mod.Oracle(out["vocab_file"], out["special_file"], None, True)
    assert ids == [orc.encode(t) for t in held]
    H.initialize(out["vocab_file"], out["special_file"], is_byte_encoder=True, merges_file_path=out["merges_file"])
    assert H.batch_encode(held) == ids


def test_bpe_train_reference_dropin(tmp_path):
    """The shim and the ctypes path write the same file, with the reference's lines on stdout."""
    import subprocess
    import sys
    from hutoken_amd import vocab_files as vf
    text = b"the quick brown fox jumps over the lazy dog. " * 40 + b"hello hello world"
    pairs, _ = train_ref.train([text], 45)
    assert 0 < len(pairs) < 45
    want = vf.raw_vocab_text(pairs, 300).encode("ascii")
    for no_shim in ("", "1"):
        home = tmp_path / ("home" + no_shim)
        home.mkdir()
        env = dict(os.environ, HOME=str(home))
        env.pop("HUTOKEN_AMD_NO_SHIM", None)
        if no_shim:
            env["HUTOKEN_AMD_NO_SHIM"] = "1"
        script = ("import hutoken_amd as H\n"
                  "text = %r\n"
                  "H.bpe_train(text, 300, 'v.txt')\n"
                  "H.bbpe_train(text, 300, 'v.txt')\n"
                  "open('%s/sp.txt', 'w').close()\n"
                  "H.initialize('%s/config/v.txt', '%s/sp.txt')\n"
                  "assert H.decode(H.encode(text)) == text\n" % (text.decode(), home, home, home))
        r = subprocess.run([sys.executable, "-c", script], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Directory created: %s/config\n" % home in r.stdout
        assert "Directory already exists: %s/config\n" % home in r.stdout
        assert "Vocab saved to: %s/config/v.txt\n" % home in r.stdout
        assert (os.stat(home / "config").st_mode & 0o777) == 0o700
        got = (home / "config" / "v.txt").read_bytes()
        assert len(got.splitlines()) == min(300, 255 + len(pairs))  # this text runs out of pairs first
        assert got.splitlines()[0] == b"0x01 == 0" and got.splitlines()[254] == b"0xFF == 254"
        assert got == want, no_shim
