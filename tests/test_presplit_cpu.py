"""The split presets gpt2, cl100k and qwen2 on the CPU: (a) the sequential restatement (presplit_ref.py) against the
`regex` module, (b) against the boundaries a tokenizer library gave (tests/golden/g13_presplit.json), (c) the rule of
csrc/hutk_presplit.h, run chunk by chunk by tests/cpu/presplit_check.cpp under the sanitizers, against the restatement,
(d) damaged table blobs are refused."""
import functools
import importlib
import json
import os
import struct
import subprocess

import pytest

import helpers as H
import presplit_cases as PC
import presplit_ref as R

PT = importlib.import_module("hutoken_amd.pretokenize")  # (the module: the package's `pretokenize` is a function)

GOLDEN = os.path.join(H.ROOT, "tests", "golden", "g13_presplit.json")


@functools.lru_cache(maxsize=None)
def _strings():
    return tuple(PC.exhaustive(5)) + tuple(PC.seeded(20000, 13))


@functools.lru_cache(maxsize=None)
def _ends(preset):
    """Match ends in characters of every string of _strings(), by the restatement."""
    return [R.split_str(s, preset) for s in _strings()]


def test_the_module_and_the_restatement_state_the_same_presets():
    assert PT.PRESETS == R.PRESETS and PT.PATTERNS == R.PATTERNS and PT.ALIASES == R.ALIASES
    assert PT.WHITE_SPACE == R.WHITE_SPACE
    assert [PT.preset_index(p) for p in ("gpt2", "cl100k", "llama3", "qwen2")] == [0, 1, 1, 2]
    with pytest.raises(ValueError):
        PT.preset_index("o200k")
    with pytest.raises(TypeError):
        PT.preset_index(1)


@pytest.mark.parametrize("preset", R.PRESETS)
def test_restatement_matches_regex(preset):
    regex = pytest.importorskip("regex")
    pat = regex.compile(R.PATTERNS[preset])
    bad = []
    for s, ends in zip(_strings(), _ends(preset)):
        got = [m.end() for m in pat.finditer(s)]
        if got != ends:
            bad.append((s, got, ends))
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:3])


def test_case_folding_of_the_contraction_letters_is_what_regex_does():
    regex = pytest.importorskip("regex")
    for c, folds in R.FOLDS.items():
        pat = regex.compile("(?i:%s)" % c)
        # (the alphabet of the cross-check, and every code point below U+3000: nothing else is a partner of an ASCII letter)
        got = {chr(x) for x in range(0x3000) if pat.fullmatch(chr(x))}
        assert got == set(folds), c


def test_restatement_matches_the_golden_boundaries():
    with open(GOLDEN, encoding="utf-8") as f:
        g = json.load(f)
    assert set(g["presets"]) == set(R.PRESETS)
    n = 0
    for preset, rows in g["presets"].items():
        for text, ends in rows:
            assert R.split_str(text, preset) == ends, (preset, text)
            n += 1
    assert n >= 3 * 250 and os.path.getsize(GOLDEN) < 500 * 1024


# ---- (c) the header ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("presplit"))
    exe = os.path.join(d, "presplit_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(H.ROOT, "hutoken_amd", "csrc"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "cpu", "presplit_check.cpp")])
    blob = os.path.join(d, "tables.bin")
    with open(blob, "wb") as f:
        f.write(PT.table_blob())
    return exe, blob, d


def _record(preset, docs, starts):
    """docs: list of bytes; starts: per document, the byte offsets of its word starts."""
    data, offs = PC.pack(docs)
    want = bytearray(len(data))
    for o, st in zip(offs, starts):
        for p in st:
            want[o + p] = 1
    return struct.pack("<II%dq" % len(offs), R.PRESETS.index(preset), len(docs), *offs) + data + bytes(want)


def _starts_of(text, ends):
    at = [0]
    for c in text:
        at.append(at[-1] + len(c.encode("utf-8", "surrogateescape")))
    return [0] + [at[e] for e in ends[:-1]] if text else []


def _run(checker, name, records, chunk):
    exe, blob, d = checker
    path = os.path.join(d, name)
    with open(path, "wb") as f:
        for r in records:
            f.write(r)
    out = subprocess.run([exe, "run", blob, path, str(chunk)], capture_output=True, text=True)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, (out.stdout + out.stderr)[-4000:]
    return out.stdout


def _grouped(docs, starts, k):
    for i in range(0, len(docs), k):
        yield docs[i:i + k], starts[i:i + k]


@pytest.mark.parametrize("preset", R.PRESETS)
def test_header_rule_on_the_regex_cases(checker, preset):
    strings, ends = _strings(), _ends(preset)
    docs = [s.encode("utf-8") for s in strings]
    starts = [_starts_of(s, e) for s, e in zip(strings, ends)]
    # every string as a batch of its own, and seven at a time as the documents of one batch (document edges everywhere)
    records = [_record(preset, [d], [st]) for d, st in zip(docs, starts)]
    records += [_record(preset, ds, sts) for ds, sts in _grouped(docs[-40000:], starts[-40000:], 7)]
    _run(checker, "regex_%s.bin" % preset, records, 64)
    _run(checker, "regex4k_%s.bin" % preset, records[-12000:], 4096)


@pytest.mark.parametrize("preset", R.PRESETS)
def test_header_rule_on_ill_formed_utf8(checker, preset):
    docs = PC.ill_formed(3000, 5) + PC.ILL_FORMED
    starts = [R.word_starts(d, preset) for d in docs]
    records = [_record(preset, [d], [st]) for d, st in zip(docs, starts)]
    records += [_record(preset, ds, sts) for ds, sts in _grouped(docs, starts, 5)]  # a cut character, then the next document
    _run(checker, "ill_%s.bin" % preset, records, 64)
    _run(checker, "ill32_%s.bin" % preset, records, 32)


@pytest.mark.parametrize("preset", R.PRESETS)
def test_header_rule_with_the_chunk_forced_down_to_64_bytes(checker, preset):
    texts = PC.carry_cases(64) + PC.edge_cases(64) + PC.edge_cases(128) + PC.seeded_texts(300, 7)
    docs = [t.encode("utf-8") for t in texts]
    starts = [R.word_starts(d, preset) for d in docs]
    records = [_record(preset, [d], [st]) for d, st in zip(docs, starts)]
    records += [_record(preset, ds, sts) for ds, sts in _grouped(docs, starts, 9)]
    out = _run(checker, "carry_%s.bin" % preset, records, 64)
    assert "cases %d " % len(records) in out
    _run(checker, "carry32_%s.bin" % preset, records, 32)
    _run(checker, "carry4k_%s.bin" % preset, records, 4096)


def test_header_rule_carries_over_real_chunks(checker):
    for preset in R.PRESETS:
        texts = PC.carry_cases(4096)[::3]
        docs = [t.encode("utf-8") for t in texts]
        _run(checker, "real_%s.bin" % preset, [_record(preset, [d], [R.word_starts(d, preset)]) for d in docs], 4096)


# ---- (d) the validator ----
def _validate(checker, blob, name):
    exe, _blob, d = checker
    path = os.path.join(d, name)
    with open(path, "wb") as f:
        f.write(blob)
    out = subprocess.run([exe, "validate", path], capture_output=True, text=True)
    assert out.returncode in (0, 3), out.stdout + out.stderr  # (anything else: a sanitizer report)
    return out.returncode == 0, out.stdout


def test_damaged_blobs_are_refused(checker):
    blob = PT.table_blob()
    assert len(blob) < 64 * 1024
    assert _validate(checker, blob, "good.bin")[0]
    words = list(struct.unpack_from("<16I", blob))

    def with_word(i, v):
        w = list(words)
        w[i] = v
        return struct.pack("<16I", *w) + blob[64:]

    damaged = {
        "empty": b"", "header only": blob[:64], "truncated": blob[:-4], "longer": blob + b"\0\0\0\0",
        "magic": with_word(0, 0x4D524E48), "version": with_word(1, 2), "size": with_word(3, words[3] + 4),
        "stage one offset past the end": with_word(4, words[3] - 8), "stage one offset odd": with_word(4, words[4] + 2),
        "stage one offset in the header": with_word(4, 8), "stage one entries": with_word(5, words[5] - 1),
        "blocks offset past the end": with_word(6, words[3]), "blocks offset huge": with_word(6, 0xFFFFFFFC),
        "no blocks": with_word(7, 0), "more blocks than there are": with_word(7, words[7] + 1),
        "too many blocks": with_word(7, 70000), "block shift": with_word(8, 8),
    }
    s1 = words[4]
    damaged["a stage-one entry past the blocks"] = blob[:s1 + 2 * 100] + struct.pack("<H", words[7]) + blob[s1 + 2 * 101:]
    for name, b in damaged.items():
        ok, out = _validate(checker, b, "damaged.bin")
        assert not ok and "refused" in out, name
