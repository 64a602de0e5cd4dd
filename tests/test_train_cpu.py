"""Training without a GPU: tests/train_ref.py against tools/train_vocab.cpp, the GPT-2 layout writer against the
committed vocabularies, and the argument checks of bpe_train / bbpe_train / train (which raise before any device call)."""
import gzip
import os
import random
import subprocess
import sys

import pytest

import helpers
import train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _cpp_pairs(exe, tmp_path, args):
    out, pf = str(tmp_path / "out.txt"), str(tmp_path / "pairs.txt")
    subprocess.run([exe, *args, out, "bytes", pf], check=False, capture_output=True)
    return [tuple(bytes.fromhex(x) for x in ln.split()) for ln in open(pf)]


def _same(cpp, pairs):
    toks = _tokens(pairs)
    assert [(toks[a], toks[b]) for a, b in pairs] == cpp


def test_train_ref_vs_cpp_synthetic(trainer_exe, tmp_path):
    from hutoken_amd import synth
    seed = 0x5EED
    cpp = _cpp_pairs(trainer_exe, tmp_path, ["2", str(seed), "2000", "2000"])
    d, o = synth.corpus("C2", 2000, seed=seed)
    raw = d.tobytes()
    pairs, _ = train_ref.train([raw[o[i]:o[i + 1]] for i in range(len(o) - 1)], 2000)
    assert len(pairs) == 2000
    _same(cpp, pairs)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_train_ref_vs_cpp_lines(trainer_exe, tmp_path, seed):
    rng = random.Random(seed)
    docs = []
    for _ in range(300):
        r = rng.random()
        if r < 0.5:
            t = helpers.random_text(rng, max_words=20).encode("utf-8")
        elif r < 0.75:
            t = helpers.random_bytes_text(rng, rng.randint(0, 40))
        else:  # tie-heavy: the same few pairs in equal numbers
            t = b" ".join(bytes([97 + rng.randrange(4), 97 + rng.randrange(4)]) for _ in range(rng.randint(1, 10)))
        docs.append(t.replace(b"\n", b" ").replace(b"\r", b" "))
    path = tmp_path / "docs.txt"
    path.write_bytes(b"".join(d + b"\n" for d in docs))
    cpp = _cpp_pairs(trainer_exe, tmp_path, ["0", str(path), "0", "600"])
    pairs, _ = train_ref.train(docs, 600)
    _same(cpp, pairs)


def _gunzip(name):
    with gzip.open(os.path.join(ROOT, "data", name), "rb") as f:
        return f.read()


def _visible_to_bytes():
    from hutoken_amd import vocab_files as vf
    return {c: b for b, c in vf.bytes_to_unicode().items()}


def test_writer_reproduces_vg():
    from hutoken_amd import vocab_files as vf
    inv = _visible_to_bytes()
    ids = {bytes([b]): b for b in range(256)}
    pairs = []
    for ln in _gunzip("vg50257_merges.txt.gz").decode("utf-8").splitlines()[1:]:
        left, right = ln.split(" ")
        lb, rb = bytes(inv[c] for c in left), bytes(inv[c] for c in right)
        pairs.append((ids[lb], ids[rb]))
        ids.setdefault(lb + rb, 256 + len(pairs) - 1)
    assert len(pairs) == 50000
    assert vf.gpt2_vocab_text(pairs).encode("utf-8") == _gunzip("vg50257_vocab.txt.gz")
    assert vf.gpt2_merges_text(pairs).encode("utf-8") == _gunzip("vg50257_merges.txt.gz")
    assert vf.gpt2_special_text() == open(os.path.join(ROOT, "data", "vg50257_special.txt"), encoding="utf-8").read()


def test_writer_reproduces_vc():
    from hutoken_amd import vocab_files as vf
    inv = _visible_to_bytes()
    lines = _gunzip("vc12257_vocab.txt.gz").decode("utf-8").splitlines()
    toks = []
    for ln in lines[256:-1]:
        hexpart = ln.split(" == ")[0]
        vis = bytes.fromhex(hexpart.replace("0x", "")).decode("utf-8")
        toks.append(bytes(inv[c] for c in vis))
    ids = {bytes([b]): b for b in range(256)}
    pairs = []
    for k, tk in enumerate(toks):  # any split into two earlier tokens
        cut = next(i for i in range(1, len(tk)) if tk[:i] in ids and tk[i:] in ids)
        pairs.append((ids[tk[:cut]], ids[tk[cut:]]))
        ids.setdefault(tk, 256 + k)
    assert len(pairs) == 12000
    assert vf.gpt2_vocab_text(pairs).encode("utf-8") == _gunzip("vc12257_vocab.txt.gz")


def test_raw_vocab_text():
    from hutoken_amd import vocab_files as vf
    txt = vf.raw_vocab_text([(97, 98), (256, 99)], 300).splitlines()
    assert len(txt) == 257 and txt[0] == "0x01 == 0" and txt[254] == "0xFF == 254"
    assert txt[255] == "0x610x62 == 255" and txt[256] == "0x610x620x63 == 256"
    assert len(vf.raw_vocab_text([(97, 98), (256, 99)], 256).splitlines()) == 256


@pytest.mark.parametrize("fn", ["bpe_train", "bbpe_train"])
def test_bpe_train_argument_checks(fn, monkeypatch, tmp_path):
    import hutoken_amd as H
    monkeypatch.setenv("HOME", str(tmp_path))
    f = getattr(H, fn)
    with pytest.raises(RuntimeError, match=r"^vocab_size must be at least 256 to encode all bytes\.$"):
        f("some text", 255, "v.txt")
    with pytest.raises(RuntimeError, match=r"^vocab_file_name file extension must be \.txt\.$"):
        f("some text", 300, "v.json")
    with pytest.raises(RuntimeError, match=r"^vocab_file_name file extension must be \.txt\.$"):
        f("some text", 300, "txt")
    with pytest.raises(TypeError):
        f(b"bytes", 300, "v.txt")
    with pytest.raises(TypeError):
        f("some text", "300", "v.txt")
    with pytest.raises(TypeError):
        f("some text", 300, None)
    with pytest.raises(TypeError):
        f("some text", 300)
    assert not (tmp_path / "config").exists()


def test_train_argument_checks(tmp_path):
    import hutoken_amd as H
    with pytest.raises(RuntimeError, match="vocab_size must be at least 256"):
        H.train(["abc"], 256, str(tmp_path), "x")  # 256 bytes + the end token do not fit
    with pytest.raises(TypeError):
        H.train(["abc"], "300", str(tmp_path), "x")
    with pytest.raises(FileNotFoundError):
        H.train(["abc"], 300, str(tmp_path / "missing"), "x")
    with pytest.raises(TypeError):
        H.train(["abc"], 300, str(tmp_path), None)
