"""Chars-mode training without a GPU: tests/train_ref_chars.py against tools/train_vocab.cpp ... chars, the
Llama-shaped writers against the committed VL files, and the mode= argument checks (which raise before any device
call)."""
import gzip
import os
import random
import subprocess
import sys

import pytest

import train_ref_chars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def trainer_exe(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_vocab
    return make_vocab.build_trainer(str(tmp_path_factory.mktemp("train_vocab")))


def cpp_chars(exe, tmp_path, args):
    """train_vocab.cpp in chars mode -> (alphabet [bytes], merges [(left bytes, right bytes)])."""
    out, pf = str(tmp_path / "out.txt"), str(tmp_path / "pairs.txt")
    subprocess.run([exe, *args, out, "chars", pf], check=False, capture_output=True)
    base = open(out).read().split("--\n")[0].split()
    return [bytes.fromhex(x) for x in base], [tuple(bytes.fromhex(x) for x in ln.split()) for ln in open(pf)]


def check_same(cpp, alphabet, pairs):
    toks = train_ref_chars.tokens(alphabet, pairs)
    assert alphabet == cpp[0]
    assert [(toks[a], toks[b]) for a, b in pairs] == cpp[1]


def test_rules_by_example():
    R = train_ref_chars
    assert R.split_chars(b"\xf0ab") == [b"\xf0ab"]
    assert R.split_chars(b"\xe2 x") == [b"\xe2\xe2\x96", b"\x81x"]
    assert R.split_chars(b" \xe2\x96\x81") == [b"\xe2\x96\x81"] * 2
    assert R.split_chars(b"\x80abcd") == [b"\x80abc", b"d"]
    assert R.split_chars(b"ab\xc3") == [b"a", b"b", b"\xc3"]
    alphabet, words, n_drop = R.symbolise({b" hi": 2, b"h\x01": 5, b"\x7f\xce\xa9": 1, b"i": 3})
    assert alphabet == [b"h", b"i", b"\xe2\x96\x81"] and n_drop == 2
    assert words == {(2, 0, 1): 2, (1,): 3}


def test_ref_vs_cpp_c5(trainer_exe, tmp_path):
    from hutoken_amd import synth
    seed = 0x564F434C
    cpp = cpp_chars(trainer_exe, tmp_path, ["5", str(seed), "3000", "2000"])
    d, o = synth.corpus("C5", 3000, seed=seed)
    raw = d.tobytes()
    alphabet, pairs, _, _ = train_ref_chars.train([raw[o[i]:o[i + 1]] for i in range(len(o) - 1)], 2000)
    assert len(pairs) == 2000
    check_same(cpp, alphabet, pairs)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ref_vs_cpp_lines(trainer_exe, tmp_path, seed):
    rng = random.Random(0xC4A5 + seed)
    docs = train_ref_chars.edge_docs(rng)
    path = tmp_path / "docs.txt"
    path.write_bytes(b"".join(d + b"\n" for d in docs))
    cpp = cpp_chars(trainer_exe, tmp_path, ["0", str(path), "0", "800"])
    alphabet, pairs, _, n_drop = train_ref_chars.train(docs, 800)
    assert n_drop > 0 and b"\xea\x80\x80" not in alphabet and b"\xe1\x9a\xa0" not in alphabet
    assert any(len(ch) == 4 for ch in alphabet) and b"\xe2\x96\x81" in alphabet
    check_same(cpp, alphabet, pairs)


def _gunzip(name):
    with gzip.open(os.path.join(ROOT, "data", name), "rb") as f:
        return f.read()


def vl_alphabet_and_pairs():
    """The alphabet and a set of merge pairs recovered out of data/vl32000_vocab.txt.gz."""
    toks = [bytes.fromhex(ln.split(" == ")[0].replace("0x", ""))
            for ln in _gunzip("vl32000_vocab.txt.gz").decode("ascii").splitlines()]
    body = toks[259:]
    A = next(i for i, tk in enumerate(body) if len(train_ref_chars.split_chars(tk)) > 1)
    alphabet = body[:A]
    ids = {tk: i for i, tk in enumerate(alphabet)}
    pairs = []
    for k, tk in enumerate(body[A:]):  # any split into two earlier tokens
        cut = next(i for i in range(1, len(tk)) if tk[:i] in ids and tk[i:] in ids)
        pairs.append((ids[tk[:cut]], ids[tk[cut:]]))
        ids.setdefault(tk, A + k)
    return alphabet, pairs


def test_llama_writers_reproduce_vl():
    from hutoken_amd import vocab_files as vf
    alphabet, pairs = vl_alphabet_and_pairs()
    assert len(alphabet) == 57 and len(pairs) == 31684
    assert vf.llama_vocab_text(alphabet, pairs).encode("ascii") == _gunzip("vl32000_vocab.txt.gz")
    assert vf.llama_special_text() == open(os.path.join(ROOT, "data", "vl32000_special.txt"), encoding="utf-8").read()
    merges = vf.llama_merges_bytes(alphabet, pairs).split(b"\n")
    assert merges[0] == b"#version: 0.2" and merges[-1] == b"" and len(merges) == len(pairs) + 2
    toks = train_ref_chars.tokens(alphabet, pairs)
    assert all(ln == toks[a] + b" " + toks[b] for ln, (a, b) in zip(merges[1:], pairs))


def test_write_llama_files(tmp_path):
    from hutoken_amd import vocab_files as vf
    alphabet = [b"a", b"b", b"\xe2\x96\x81"]
    paths = vf.write_llama_files(str(tmp_path), "t", alphabet, [(2, 0), (3, 1)])
    lines = open(paths["vocab_file"]).read().splitlines()
    assert len(lines) == 259 + 3 + 2
    assert lines[0] == "0x3C0x750x6E0x6B0x3E == 0" and lines[258] == "0x3C0x300x780x460x460x3E == 258"
    assert lines[261] == "0xE20x960x81 == 261" and lines[263] == "0xE20x960x810x610x62 == 263"
    assert open(paths["merges_file"], "rb").read() == b"#version: 0.2\n\xe2\x96\x81 a\n\xe2\x96\x81a b\n"
    assert open(paths["special_file"], "rb").read() == open(os.path.join(ROOT, "data", "vl32000_special.txt"),
                                                              "rb").read()


def test_mode_argument_checks(tmp_path):
    """Every check raises before a device is opened (this box may have none: a device error would be RuntimeError)."""
    import hutoken_amd as H
    for bad in ("words", "CHARS", None, 1, b"chars"):
        with pytest.raises(ValueError, match="mode must be 'bytes' or 'chars'"):
            H.Trainer(mode=bad)
        with pytest.raises(ValueError, match="mode must be 'bytes' or 'chars'"):
            H.train(["abc"], 300, str(tmp_path), "x", mode=bad)
    with pytest.raises(RuntimeError, match="at least 259"):
        H.train(["abc"], 258, str(tmp_path), "x", mode="chars")
    with pytest.raises(FileNotFoundError):
        H.train(["abc"], 300, str(tmp_path / "missing"), "x", mode="chars")
    with pytest.raises(TypeError):
        H.train(["abc"], "300", str(tmp_path), "x", mode="chars")
    assert os.listdir(tmp_path) == []

