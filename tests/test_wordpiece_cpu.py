"""WordPiece without a GPU: (a) the restatement tests/wordpiece_ref.py on the hand-worked cases of the rule and on the
goldens that `tokenizers` wrote, (b) the argument checks and refusals of hutoken_amd.WordPiece that need no device,
(c) the table blob: its validator on damaged blobs, its classes and mappings against the restatement, the capacity bound
on every code point, (d) the rule as the kernels run it -- hutoken_amd/csrc/hutk_wordpiece.h, run chunk by chunk by
tests/cpu/wordpiece_check.cpp under the sanitizers -- against the restatement, id for id."""
import os
import struct
import subprocess
import unicodedata

import numpy as np
import pytest

import helpers as H
import wordpiece_cases as WC
import wordpiece_ref as R
import hutoken_amd
from hutoken_amd import wordpiece as WT

SMALL = ["[UNK]", "a", "b", "ab", "##b", "##c", "un", "##aff", "##able", "aff", ",", "\u4e2d", "i\u0307", "i", "\u03b1\u03c3", "\ud55c",
         "\u1112", "##\u1161", "##\u11ab", "e", "##e"]


def _ids(vocab, text, **flags):
    return R.encode(vocab, text, **flags)[0]


# ---- (a) the restatement ----
def test_hand_worked_normaliser_cases():
    n = R.normalize
    assert n("a\u200bb") == "ab" and R.split(n("a\u200bb")) == ["ab"]                   # a dropped character joins its neighbours
    assert R.split(n("a\u0378b")) == ["a\u0378b"]                                       # Cn is not dropped
    assert n("a\u00a0\u2028\u2029b\u3000") == "a   b "                                  # White_Space becomes ' '
    assert n("a\x0bb\x0cc\x85d") == "abcd"                                            # Cc: dropped, not spaces
    assert n("a\tb\nc\rd") == "a b c d"
    assert n("\x00\ufffda") == "a"
    assert n("\u0391\u03a3", strip_accents=False) == "\u03b1\u03c3"                     # no final-sigma rule
    assert n("\u0130", strip_accents=False) == "i\u0307" and n("\u0130") == "i"
    assert n("\ud55c") == "\u1112\u1161\u11ab"                                          # Hangul syllables become jamo
    assert n("\u4e2da") == " \u4e2d a" and n("\u4e2d", handle_chinese_chars=False) == "\u4e2d"
    assert n("\U0002b820") == "\U0002b820" and n("\U0002b920") == " \U0002b920 "        # the sixth range starts at 2B920
    assert n("\u00c9", lowercase=False) == "\u00c9" and n("\u00c9", lowercase=False, strip_accents=True) == "E"
    assert n("\udc80A") == "\udc80a"                                                    # an ill-formed byte stays


def test_hand_worked_split_and_match_cases():
    v = R.Vocab(SMALL)
    assert R.split("ab,c  d!") == ["ab", ",", "c", "d", "!"]
    assert _ids(v, "ab") == [3] and _ids(v, "abc") == [3, 5] and _ids(v, "unaffable") == [6, 7, 8]
    assert _ids(R.Vocab(["[UNK]", "a"]), "aaa") == [0]                                  # "##a" is missing: the word is unk
    assert _ids(v, "abx") == [0] and _ids(v, "") == [] and _ids(v, " \n ") == []
    assert _ids(v, "a" * 101) == [0]
    assert _ids(R.Vocab(["[UNK]", "a", "##a"]), "a" * 100) == [1] + [2] * 99
    assert _ids(R.Vocab(["[UNK]", "a", "##a"]), "a" * 101) == [0]
    assert _ids(R.Vocab(["[UNK]", "éé"], max_input_chars_per_word=2), "éé", lowercase=False) == [1]  # characters, not bytes
    assert R.Vocab(["a", "b", "a"], unk_token="b").ids == {"b": 1, "a": 2}               # the later id wins
    assert R.encode(v, "ab, abc") == ([3, 10, 3, 5], [0, 1, 2, 2])
    assert _ids(v, "a中b") == [1, 11, 2]


def test_restatement_matches_the_goldens():
    g = WC.golden_docs()
    lines = WC.golden_vocab()
    assert 2000 < len(lines) < 5000 and lines.count("ház") == 2
    assert set(g["settings"]) == set(WC.SETTINGS) and len(g["texts"]) >= 300
    for name, s in g["settings"].items():
        v = R.Vocab(lines)
        multi = 0
        for t, ids, wids in zip(g["texts"], s["ids"], s["word_ids"]):
            assert R.encode(v, t, **WC.SETTINGS[name]) == (ids, wids), (name, t)
            multi += len(ids) > len(set(wids))
        assert multi > 100  # (most documents hold words of several pieces)
        assert any(v.unk in ids for ids in s["ids"])


# ---- (b) the Python surface, before any device call ----
def test_wordpiece_refuses_bad_arguments_without_a_device():
    WP = hutoken_amd.WordPiece
    wp = WP(["[UNK]", "a", "##b", "a"])
    assert wp.vocab_size == 4 and wp.token_to_id("a") == 3 and wp.id_to_token(2) == "##b"
    assert wp.token_to_id("zz") is None and wp.id_to_token(9) is None
    for bad, exc in (("[UNK]", TypeError), (None, TypeError), ([], ValueError), (["[UNK]", 3], TypeError), (["[UNK]", ""], ValueError),
                     (["a"], ValueError)):
        with pytest.raises(exc):
            WP(bad)
    with pytest.raises(ValueError, match="16 bytes"):
        WP(["[UNK]"], continuing_subword_prefix="#" * 17)
    with pytest.raises(ValueError):
        WP(["[UNK]"], max_input_chars_per_word=-1)
    with pytest.raises(TypeError):
        WP(["[UNK]"], max_input_chars_per_word=1.5)
    with pytest.raises(TypeError):
        WP(["[UNK]"], lowercase=1)
    with pytest.raises(TypeError):
        WP(["[UNK]"], strip_accents="yes")
    with pytest.raises(TypeError):
        WP(["[UNK]"], unk_token=0)
    with pytest.raises(TypeError):
        wp.batch_encode("text")
    with pytest.raises(TypeError):
        wp.encode(["text"])
    with pytest.raises(TypeError):
        wp.encode_packed_device(np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.int64))
    assert "WordPiece" in hutoken_amd.__all__ and "WordPiece" in hutoken_amd.__doc__


def test_from_file_reads_one_token_a_line(tmp_path):
    p = tmp_path / "vocab.txt"
    p.write_bytes("[UNK]\na\r\n##é\n".encode("utf-8"))
    wp = hutoken_amd.WordPiece.from_file(str(p), lowercase=False)
    assert wp.vocab_size == 3 and wp.token_to_id("a") == 1 and wp.token_to_id("##é") == 2
    assert wp._flags == WT.CLEAN_TEXT | WT.CJK_CHARS


def test_flags_follow_the_options():
    assert WT.flags_of() == 15 and WT.flags_of(lowercase=False) == 3 and WT.flags_of(strip_accents=False) == 11
    assert WT.flags_of(lowercase=False, strip_accents=True, clean_text=False, handle_chinese_chars=False) == 4


# ---- (c) the tables ----
def test_blob_states_the_classes_and_mappings_of_the_restatement():
    blob = WT.table_blob()
    assert WT.validate_blob(blob) is None and len(blob) < 256 * 1024
    head = struct.unpack_from("<32I", blob, 0)
    assert head[0] == WT.MAGIC and head[1] == 1 and head[3] == len(blob)
    uv = [int(x) for x in unicodedata.unidata_version.split(".")]
    assert head[2] == uv[0] << 16 | uv[1] << 8 | uv[2]
    stage1 = np.frombuffer(blob, dtype="<u2", count=head[5], offset=head[4]).astype(np.int64)
    words = np.frombuffer(blob, dtype="<u4", count=head[7] << 7, offset=head[6]).reshape(head[7], 128)[stage1].reshape(-1)
    for c in range(0x110000):
        if 0xD800 <= c < 0xE000:
            continue
        ch, w = chr(c), int(words[c])
        plain = WT.SPACE if R.is_space(ch) else WT.PUNCT if R.is_punct(ch) else WT.MARK if unicodedata.category(ch) == "Mn" else \
            WT.CJK if R.is_cjk(ch) else WT.WORD
        assert (w >> 24) & 7 == plain, hex(c)
        assert w & 7 == (WT.DROPPED if R.is_dropped(ch) else plain), hex(c)
        if (w >> 3) & 0x1FFFFF or w >> 27:
            assert WT.lower_of(blob, c) == ch.lower(), hex(c)
        else:
            assert ch.lower() == ch, hex(c)


def test_capacity_bound_holds_on_every_code_point():
    """An id is at least one character of the normalised text that is no space, so characters out per byte in bounds the
    ids.  Dropping, mapping to a space and (CJK) adding spaces put out no further character that can be part of a word;
    only NFD and the lower-case mapping can, so the restatement runs on every code point that either changes."""
    head = struct.unpack_from("<32I", WT.table_blob(), 0)
    seen = 0
    for c in range(0x110000):
        if 0xD800 <= c < 0xE000:
            continue
        ch = chr(c)
        if unicodedata.normalize("NFD", ch) == ch and ch.lower() == ch:
            continue
        seen += 1
        src = len(ch.encode("utf-8"))
        for s in range(4):
            out = R.normalize(ch, lowercase=bool(s & 1), strip_accents=bool(s & 2))
            assert len([x for x in out if not R.is_space(x)]) <= head[16 + s] * src, (hex(c), s)
            folded = len(out.replace(" ", "").encode("utf-8")) if R.is_cjk(ch) else len(out.encode("utf-8"))
            assert 16 * folded <= head[20 + s] * src, (hex(c), s)
    assert seen > 10000 and list(head[16:20]) == [1, 1, 1, 1]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wordpiece"))
    exe = os.path.join(d, "wordpiece_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(H.ROOT, "hutoken_amd", "csrc"), "-o", exe,
                           os.path.join(H.ROOT, "tests", "cpu", "wordpiece_check.cpp")])
    blob = os.path.join(d, "tables.bin")
    with open(blob, "wb") as f:
        f.write(WT.table_blob())
    return exe, blob, d


def _validate(checker, blob, name):
    exe, _good, d = checker
    path = os.path.join(d, name)
    with open(path, "wb") as f:
        f.write(blob)
    out = subprocess.run([exe, "validate", path], capture_output=True, text=True)
    assert out.returncode in (0, 3), out.stdout + out.stderr  # (anything else: a sanitizer report)
    assert (out.returncode == 0) == (WT.validate_blob(blob) is None), name
    return out.returncode == 0


def test_damaged_blobs_are_refused(checker):
    blob = WT.table_blob()
    assert _validate(checker, blob, "good.bin")
    head = list(struct.unpack_from("<32I", blob, 0))

    def with_head(i, v):
        h = list(head)
        h[i] = v
        return struct.pack("<32I", *h) + blob[128:]

    def with_word(at, v):
        return blob[:at] + struct.pack("<I", v) + blob[at + 4:]

    bad = [blob[:64], blob[:-4], blob[:-1], blob + b"\0\0\0\0", b"", with_head(0, 0), with_head(1, 2), with_head(3, len(blob) - 4),
           with_head(4, len(blob) - 8), with_head(4, 130), with_head(5, 10), with_head(6, len(blob)), with_head(7, 70000),
           with_head(7, head[7] + 1), with_head(8, len(blob) + 4), with_head(9, 40), with_head(9, 0), with_head(10, 8),
           with_head(16, 0), with_head(17, 9), with_head(20, 8), with_head(23, 100),
           blob[:head[4]] + struct.pack("<H", head[7]) + blob[head[4] + 2:],          # a stage-one entry past the blocks
           with_word(head[6] + 4 * 65, 6),                                            # a class that does not exist
           with_word(head[6] + 4 * 65, 7 << 24),
           with_word(head[6] + 4 * 65, (0x110000 - 65) << 3),                             # a mapping that is no code point
           with_word(head[6] + 4 * 65, 31 << 27),                                     # a second character past the table
           with_word(head[8] + 4, 0x110000)]
    for i, b in enumerate(bad):
        assert not _validate(checker, b, "bad%d.bin" % i), i


# ---- (d) the header's rule, chunk by chunk ----
def _fold(checker, mode, pad, chunk, data, offs, tag):
    exe, blob, d = checker
    case, out = os.path.join(d, tag + ".fold"), os.path.join(d, tag + ".folded")
    with open(case, "wb") as f:
        f.write(struct.pack("<5q", mode, 1 if pad else 0, chunk, len(offs) - 1, len(data)) + offs.tobytes() + data.tobytes())
    r = subprocess.run([exe, "fold", blob, case, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(out, "rb").read()
    total = struct.unpack_from("<q", raw, 0)[0]
    oo = np.frombuffer(raw, dtype="<i8", count=len(offs), offset=8).copy()
    return np.frombuffer(raw, dtype=np.uint8, count=total, offset=8 + 8 * len(offs)).copy(), oo


def run_header(checker, lines, docs, chunk, tag, unk="[UNK]", prefix="##", max_chars=100, **options):
    """The orchestration of hutk_wordpiece_encode_batch_device on the CPU: fold (around NFD with strip_accents), split
    and match -> (ids, offsets, word_ids) as lists."""
    exe, blob, d = checker
    flags = WT.flags_of(**options)
    data, offs = WC.pack(docs)
    lower = 4 if flags & WT.LOWERCASE else 0
    if flags & WT.STRIP_ACCENTS:
        if flags & WT.CLEAN_TEXT:
            data, offs = _fold(checker, 1, True, chunk, data, offs, tag + "a")
            assert len(data) == sum(map(len, docs))
        raw = data.tobytes()
        nfd = [R._nfd(R.text_of(raw[offs[i]:offs[i + 1]])).encode("utf-8", "surrogateescape") for i in range(len(docs))]
        data, offs = WC.pack(nfd)
        data, offs = _fold(checker, 2 | lower, False, chunk, data, offs, tag + "b")
    else:
        data, offs = _fold(checker, (1 if flags & WT.CLEAN_TEXT else 0) | lower, False, chunk, data, offs, tag + "b")
    vb = [t.encode("utf-8") for t in lines]
    vdata, voffs = WC.pack(vb)
    case, out = os.path.join(d, tag + ".match"), os.path.join(d, tag + ".ids")
    with open(case, "wb") as f:
        f.write(struct.pack("<9q", flags, max_chars, chunk, len(vb), len(vdata), len(unk.encode()), len(prefix.encode()),
                            len(offs) - 1, len(data)))
        f.write(voffs.tobytes() + vdata.tobytes() + unk.encode() + prefix.encode() + offs.tobytes() + data.tobytes())
    r = subprocess.run([exe, "match", blob, case, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(out, "rb").read()
    total = struct.unpack_from("<q", raw, 0)[0]
    oo = np.frombuffer(raw, dtype="<i8", count=len(offs), offset=8).tolist()
    at = 8 + 8 * len(offs)
    ids = np.frombuffer(raw, dtype="<i4", count=total, offset=at).tolist()
    wids = np.frombuffer(raw, dtype="<i4", count=total, offset=at + 4 * total).tolist()
    return ids, oo, wids


ILL_FORMED = [b"\x80", b"a\x80b", b"\xc3", b"ab\xe4\xb8", b"\xe4\xb8", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
              b"\xf0\x9f\x98", b"x\xf0\x9f\x98", b"\xa9 a", b"\xc3\xc3\xa9", b"a\xffb, c", b"\xe4\xb8\xad\xe4\xb8", b"\x80\x80\x80\x80"]


@pytest.mark.parametrize("setting", sorted(WC.SETTINGS))
@pytest.mark.parametrize("chunk", [16, 64, 4096])
def test_header_rule_matches_the_restatement(checker, setting, chunk):
    lines = WC.golden_vocab()
    opts = WC.SETTINGS[setting]
    docs = [t.encode("utf-8") for t in WC.texts(120, 5 + chunk, 0, 30)] + ILL_FORMED + [b"", b"a" * 100, b"a" * 101, "é".encode() * 101,
            ("meg" * 40).encode(), b"x" * 5000, b"..." * 30, b""]
    # documents that end in a sequence cut short, in front of one that starts with continuation bytes
    docs += [b"ab\xe4\xb8", b"\xad cd", b"\xc3", b"\xa9"]
    want = WC.encode_docs(R.Vocab(lines), docs, **opts)
    got = run_header(checker, lines, docs, chunk, "%s%d" % (setting, chunk), **opts)
    assert got == want


def test_header_rule_with_other_options(checker):
    lines = SMALL + ["##a", "x" * 30, "##" + "y" * 30 + "é", "##" + "y" * 30 + "e", "y"]
    docs = [t.encode("utf-8") for t in WC.texts(60, 3, 0, 20)] + ["unaffable ab abc aaa a中b 한국 İ ΑΣ".encode(), b"a\x0bb\x85 c\xc2\x85d",
            ("y" * 31 + "é y" + "y" * 30 + "e y" + "y" * 30 + "x").encode()]
    for k, opts in enumerate((dict(clean_text=False), dict(handle_chinese_chars=False), dict(lowercase=False, strip_accents=True),
                              dict(lowercase=True, strip_accents=False, clean_text=False, handle_chinese_chars=False))):
        for max_chars in (1, 3, 100):
            v = R.Vocab(lines, max_input_chars_per_word=max_chars)
            assert run_header(checker, lines, docs, 32, "o%d_%d" % (k, max_chars), max_chars=max_chars, **opts) == \
                WC.encode_docs(v, docs, **opts), (opts, max_chars)
    v = R.Vocab(lines, unk_token="a", prefix="ab")
    assert run_header(checker, lines, docs, 16, "p", unk="a", prefix="ab") == WC.encode_docs(v, docs)


def test_header_refuses_what_the_rule_refuses(checker):
    exe, blob, d = checker
    for k, (lines, unk, prefix) in enumerate(((["a", ""], "a", "##"), (["a"], "b", "##"), (["a"], "a", "#" * 17))):
        vb = [t.encode() for t in lines]
        vdata, voffs = WC.pack(vb)
        case = os.path.join(d, "refuse%d" % k)
        with open(case, "wb") as f:
            f.write(struct.pack("<9q", 15, 100, 16, len(vb), len(vdata), len(unk), len(prefix), 0, 0))
            f.write(voffs.tobytes() + vdata.tobytes() + unk.encode() + prefix.encode() + struct.pack("<q", 0))
        r = subprocess.run([exe, "match", blob, case, case + ".out"], capture_output=True, text=True)
        assert r.returncode == 5 and "refused" in r.stderr, r.stdout + r.stderr
