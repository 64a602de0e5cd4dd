"""The GPU normaliser without a GPU: its tables (hutoken_amd/normalize.py) against unicodedata; the code the kernels
run (csrc/hutk_norm.h: UTF-8 rule, segment rule, per-segment normaliser, with the real chunk size) on the CPU under
AddressSanitizer and UBSan (tests/cpu/norm_check.cpp, a child process) against tests/norm_ref.py, byte for byte, for
all four forms; the blob validator on damaged blobs; the argument checks of the Python surface; hf.export's key."""
import importlib
import json
import os
import struct
import subprocess
import unicodedata

import numpy as np
import pytest

import helpers as H
import norm_ref as R

tables = importlib.import_module("hutoken_amd.normalize")  # (the package's `normalize` is the list-form function)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("norm")), "norm_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I" + os.path.join(H.ROOT, "hutoken_amd", "csrc"), "-o", out,
                           os.path.join(H.ROOT, "tests", "cpu", "norm_check.cpp")])
    return out


@pytest.fixture(scope="module")
def blob_file(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("blob")), "tables.bin")
    with open(path, "wb") as f:
        f.write(tables.table_blob())
    return path


def _clean(r):
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def _chunk(exe):
    r = subprocess.run([exe, "chunk"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0
    return int(r.stdout)


def _run(exe, blob_file, tmp_path, docs, tag):
    """the batch through norm_check under all four forms == the reference: text, offsets and changed flags"""
    data, offs = R.pack(docs)
    case, prefix = os.path.join(str(tmp_path), tag + ".case"), os.path.join(str(tmp_path), tag + ".out")
    with open(case, "wb") as f:
        f.write(struct.pack("<qq", len(docs), len(data)))
        f.write(offs.tobytes())
        f.write(data.tobytes())
    r = subprocess.run([exe, "run", blob_file, case, prefix], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    _clean(r)
    n = len(docs)
    for fi, form in enumerate(R.FORMS):
        raw = open("%s.%d" % (prefix, fi), "rb").read()
        total = struct.unpack_from("<q", raw)[0]
        oo = np.frombuffer(raw, dtype=np.int64, count=n + 1, offset=8)
        ch = np.frombuffer(raw, dtype=np.uint8, count=n, offset=8 + 8 * (n + 1))
        out = np.frombuffer(raw, dtype=np.uint8, count=total, offset=8 + 8 * (n + 1) + n)
        rd, ro, rc = R.reference(form, docs)
        assert np.array_equal(oo, ro), (tag, form)
        assert np.array_equal(ch, rc), (tag, form)
        if not np.array_equal(out, rd):
            bounds = ro.tolist()
            for i in range(n):
                assert out[bounds[i]:bounds[i + 1]].tobytes() == rd[bounds[i]:bounds[i + 1]].tobytes(), (tag, form, i, docs[i][:64])
        os.remove("%s.%d" % (prefix, fi))
    os.remove(case)


def test_every_scalar_value_as_a_document(exe, blob_file, tmp_path):
    docs = R.scalar_docs()
    assert len(docs) == 1112064
    _run(exe, blob_file, tmp_path, docs, "scalars")


def test_every_scalar_value_wrapped(exe, blob_file, tmp_path):
    _run(exe, blob_file, tmp_path, R.wrapped_docs(), "wrapped")


def test_random_documents(exe, blob_file, tmp_path):
    docs = R.random_docs()
    assert len(docs) == 20000 and all(1 <= len(d.decode("utf-8")) <= 12 for d in docs)
    _run(exe, blob_file, tmp_path, docs, "random")


def test_ill_formed_bytes(exe, blob_file, tmp_path):
    docs = R.byte_fuzz_docs()
    assert len(docs) == 2000 and max(map(len, docs)) == 40 and min(map(len, docs)) == 0
    _run(exe, blob_file, tmp_path, docs, "bytes")
    _run(exe, blob_file, tmp_path, R.cut_docs(_chunk(exe)), "cut")


def test_named_cases(exe, blob_file, tmp_path):
    C = _chunk(exe)
    for s, want in zip(R.NAMED, R.NAMED_NFC):
        assert R.norm_doc("NFC", s.encode("utf-8")) == want.encode("utf-8"), s
    assert len(R.norm_doc("NFKC", "\ufdfa".encode("utf-8"))) == 33 == len(R.norm_doc("NFKD", "\ufdfa".encode("utf-8")))
    _run(exe, blob_file, tmp_path, R.edge_docs(C), "edges")
    for i, batch in enumerate(R.boundary_batches(C)):
        _run(exe, blob_file, tmp_path, batch, "bound%d" % i)
    _run(exe, blob_file, tmp_path, R.long_run_docs(C), "long")
    _run(exe, blob_file, tmp_path, [], "none")
    _run(exe, blob_file, tmp_path, [b""] * 5, "empty")
    _run(exe, blob_file, tmp_path, [b""] * 500 + [b"o\xcc\x8b"] + [b""] * 500, "around")


def test_table_facts_against_unicodedata():
    facts = tables.table_facts()
    assert facts["unidata_version"] == unicodedata.unidata_version
    assert facts["first_unstable"] == [0x300, 0xC0, 0xA0, 0xA0]
    assert facts["first_lead"] == [0xCC, 0xC3, 0xC2, 0xC2]
    assert facts["max_expansion"] == [3, 3, 11, 11]
    ccc = facts["ccc"]
    assert len(ccc) == 0x110000
    assert all(ccc[c] == unicodedata.combining(chr(c)) for c in range(0x110000))
    pairs = facts["pairs"]
    assert len(pairs) > 900
    for (a, b), c in pairs.items():
        assert unicodedata.normalize("NFC", chr(a) + chr(b)) == chr(c), (a, b, c)
    # ... and the blob says the same: the ccc of every code point through the two-stage index, the header's facts
    blob = tables.table_blob()
    head = struct.unpack_from("<32I", blob)
    assert head[0] == tables.MAGIC and head[1] == tables.VERSION and head[3] == len(blob)
    assert list(head[16:20]) == [0xCC, 0xC3, 0xC2, 0xC2] and list(head[20:24]) == [3, 3, 11, 11]
    stage1 = np.frombuffer(blob, dtype=np.uint16, count=head[5], offset=head[4]).astype(np.int64)
    props = np.frombuffer(blob, dtype=np.uint32, count=head[7] * 256, offset=head[6])
    cps = np.arange(0x110000, dtype=np.int64)
    w0 = props[((stage1[cps >> 7] << 7) | (cps & 127)) * 2]
    assert np.array_equal((w0 & 0xFF).astype(np.uint8), np.frombuffer(ccc, dtype=np.uint8))
    slots = np.frombuffer(blob, dtype=np.uint32, count=head[11] * 4, offset=head[10]).reshape(-1, 4)
    filled = slots[slots[:, 0] != tables.EMPTY]
    assert len(filled) == head[12] == len(pairs)
    assert {(int(a), int(b)): int(c) for a, b, c, _z in filled} == pairs


def test_building_the_tables_is_quick():
    import time
    t0 = time.perf_counter()
    tables._build()
    assert time.perf_counter() - t0 < 10.0  # (about a second; the bound only catches a return to per-code-point calls)


def test_blob_writer(tmp_path):
    import sys
    path = os.path.join(str(tmp_path), "t.bin")
    r = subprocess.run([sys.executable, "-W", "ignore", "-m", "hutoken_amd.normalize", "--write", path], capture_output=True, text=True, cwd=H.ROOT)
    assert r.returncode == 0, r.stderr
    assert open(path, "rb").read() == tables.table_blob()


def test_damaged_blobs_are_refused(exe, tmp_path):
    good = tables.table_blob()
    head = list(struct.unpack_from("<32I", good))

    def with_word(at, value):
        b = bytearray(good)
        struct.pack_into("<I", b, at, value)
        return bytes(b)

    stage1, props, decomp, pairs = head[4], head[6], head[8], head[10]
    # a property word 1 that is not zero, to corrupt a decomposition index: U+00C0's
    blk = struct.unpack_from("<H", good, stage1 + 2 * (0xC0 >> 7))[0]
    w1_at = props + 8 * ((blk << 7) | (0xC0 & 127)) + 4
    idx = struct.unpack_from("<I", good, w1_at)[0] & 0xFFFF
    assert idx
    cases = {
        "truncated": good[:-5],
        "header only": good[:64],
        "empty": b"",
        "magic": with_word(0, 0x12345678),
        "version": with_word(4, 99),
        "stage1 offset": with_word(16, len(good) - 64),
        "stage1 entry": good[:stage1] + b"\xff\xff" + good[stage1 + 2:],
        "props offset": with_word(24, len(good) + 8),
        "props blocks": with_word(28, head[7] + 50000),
        "decomposition index": with_word(w1_at, 0xFFF0FFF0),
        "decomposition length": with_word(decomp + 4 * idx, 200),
        "decomposition code point": with_word(decomp + 4 * (idx + 1), 0x1FFFFF),
        "decomposition offset": with_word(32, len(good) - 8),
        "pair offset": with_word(40, 6),
        "pair slots": with_word(44, head[11] * 2),
        "pair slots not a power of two": with_word(44, head[11] - 1),
        "pair count": with_word(48, head[12] + 1),
        "pair code point": with_word(pairs + 16 * int(np.flatnonzero(np.frombuffer(good, dtype=np.uint32, count=head[11] * 4, offset=pairs)[::4] != tables.EMPTY)[0]) + 8, 0x7FFFFFFF),
        "lead byte": with_word(4 * 16, 0x41),
    }
    ok = subprocess.run([exe, "validate", _write(tmp_path, "good", good)], capture_output=True, text=True, env=ENV)
    assert ok.returncode == 0, ok.stderr
    for name, blob in cases.items():
        r = subprocess.run([exe, "validate", _write(tmp_path, "bad", blob)], capture_output=True, text=True, env=ENV)
        _clean(r)
        assert r.returncode == 3 and r.stderr.startswith("refused: normaliser tables: "), (name, r.returncode, r.stderr[-500:])


def _write(tmp_path, name, blob):
    path = os.path.join(str(tmp_path), name + ".bin")
    with open(path, "wb") as f:
        f.write(blob)
    return path


def test_library_refuses_a_damaged_blob_before_any_device():
    from hutoken_amd import _capi
    with pytest.raises(ValueError, match="normaliser tables"):
        _capi.Normalizer(tables.table_blob()[:-4])
    with pytest.raises(ValueError, match="wrong magic"):
        _capi.Normalizer(b"\0" * 4096)
    assert _capi.norm_chunk_bytes() == 4096


class _FakeTensor:
    """enough of a tensor for the argument checks: they come before anything touches torch or the library"""

    def __init__(self, dtype, cuda=True, dim=1, device="cuda:0", n=4):
        self.dtype, self.is_cuda, self._dim, self.device, self._n = dtype, cuda, dim, device, n

    def data_ptr(self):
        raise AssertionError("the library was reached")

    def dim(self):
        return self._dim

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n


def test_argument_errors_come_before_the_library(monkeypatch):
    import hutoken_amd
    from hutoken_amd import _capi

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_capi, "load", boom)
    good_b, good_o = _FakeTensor("torch.uint8"), _FakeTensor("torch.int64")
    for form, exc in (("nfc", ValueError), ("NFX", ValueError), ("", ValueError), (None, TypeError), (0, TypeError), (b"NFC", TypeError)):
        with pytest.raises(exc, match="form must be one of"):
            hutoken_amd.normalize_packed_device(good_b, good_o, form)
        with pytest.raises(exc, match="form must be one of"):
            hutoken_amd.normalize(["a"], form)
    with pytest.raises(TypeError, match="must be a torch tensor"):
        hutoken_amd.normalize_packed_device(b"abc", good_o)
    with pytest.raises(TypeError, match="must be a torch tensor"):
        hutoken_amd.normalize_packed_device(good_b, [0, 3])
    with pytest.raises(TypeError, match="dtype uint8"):
        hutoken_amd.normalize_packed_device(_FakeTensor("torch.int32"), good_o)
    with pytest.raises(TypeError, match="dtype int64"):
        hutoken_amd.normalize_packed_device(good_b, _FakeTensor("torch.int32"))
    with pytest.raises(ValueError, match="on the GPU"):
        hutoken_amd.normalize_packed_device(_FakeTensor("torch.uint8", cuda=False), good_o)
    with pytest.raises(ValueError, match="one-dimensional"):
        hutoken_amd.normalize_packed_device(_FakeTensor("torch.uint8", dim=2), good_o)
    with pytest.raises(ValueError, match="same device"):
        hutoken_amd.normalize_packed_device(good_b, _FakeTensor("torch.int64", device="cuda:1"))
    with pytest.raises(ValueError, match="at least one entry"):
        hutoken_amd.normalize_packed_device(good_b, _FakeTensor("torch.int64", n=0))
    with pytest.raises(TypeError, match="n_out"):
        hutoken_amd.normalize_packed_device(good_b, good_o, n_out=1.5)
    with pytest.raises(ValueError, match="n_out"):
        hutoken_amd.normalize_packed_device(good_b, good_o, n_out=-1)
    with pytest.raises(TypeError, match="list of strings"):
        hutoken_amd.normalize("abc")
    # normalize= of the list-form entry points: checked first, whatever else is wrong
    packer = hutoken_amd.SequencePacker.__new__(hutoken_amd.SequencePacker)
    calls = [lambda f: hutoken_amd.batch_encode_padded(["a"], 8, normalize=f),
             lambda f: hutoken_amd.batch_encode_windows(["a"], 8, normalize=f),
             lambda f: packer.add_texts(["a"], normalize=f),
             lambda f: hutoken_amd.batch_encode_special(["a"], normalize=f),
             lambda f: hutoken_amd.batch_encode_fallback(["a"], normalize=f)]
    for call in calls:
        with pytest.raises(ValueError, match="form must be one of"):
            call("NFKX")
        with pytest.raises(TypeError, match="form must be one of"):
            call(3)


def test_normalize_none_takes_the_old_path(monkeypatch):
    """normalize=None (and the keyword left out) never reaches normalize_packed_device: _encode_texts gets None"""
    import hutoken_amd
    seen = []

    def fake_encode_texts(kind, texts, flags=0, with_text=False, normalize=None):
        seen.append((kind, normalize))
        raise KeyError("stop here")
    monkeypatch.setattr(hutoken_amd, "_encode_texts", fake_encode_texts)
    monkeypatch.setattr(hutoken_amd, "_ctx", object())
    monkeypatch.setattr(hutoken_amd, "normalize_packed_device", lambda *a, **k: pytest.fail("normalised"))
    packer = hutoken_amd.SequencePacker.__new__(hutoken_amd.SequencePacker)
    for call in (lambda **k: hutoken_amd.batch_encode_padded(["a"], 8, **k), lambda **k: hutoken_amd.batch_encode_windows(["a"], 8, **k),
                 lambda **k: packer.add_texts(["a"], **k), lambda **k: hutoken_amd.batch_encode_special(["a"], **k),
                 lambda **k: hutoken_amd.batch_encode_fallback(["a"], **k)):
        for kw in ({}, {"normalize": None}, {"normalize": "NFKC"}):
            with pytest.raises(KeyError):
                call(**kw)
    kinds = ["plain", "plain", "plain", "special", "fallback"]
    assert seen == [(k, f) for k in kinds for f in (None, None, "NFKC")]
    assert "normalize_packed_device" in hutoken_amd.__all__ and "normalize" in hutoken_amd.__all__


class _StubBackend:
    def __init__(self, normalizer):
        self._js = {"normalizer": normalizer, "model": {}}

    def to_str(self):
        return json.dumps(self._js)


class _StubTokenizer:
    def __init__(self, normalizer):
        self.backend_tokenizer = _StubBackend(normalizer)


@pytest.mark.parametrize("node, want", [
    ({"type": "NFC"}, "NFC"),
    ({"type": "NFKD"}, "NFKD"),
    ({"type": "Sequence", "normalizers": [{"type": "NFKC"}]}, "NFKC"),
    ({"type": "Sequence", "normalizers": [{"type": "Replace", "pattern": {"String": " "}, "content": "_"}, {"type": "NFKC"}]}, "NFKC"),
    ({"type": "Sequence", "normalizers": [{"type": "NFD"}, {"type": "NFKC"}]}, None),
    ({"type": "Sequence", "normalizers": []}, None),
    ({"type": "Lowercase"}, None),
    (None, None),
])
def test_hf_normalizer_form(node, want):
    from hutoken_amd import hf
    assert hf.normalizer_form(_StubTokenizer(node)) == want


def test_hf_export_reports_the_normalizer(monkeypatch, tmp_path):
    from hutoken_amd import hf

    class Tok(_StubTokenizer):
        def save_pretrained(self, folder):
            pass

        def tokenize(self, text):
            return [text]

    tok = Tok({"type": "Sequence", "normalizers": [{"type": "NFKC"}]})
    monkeypatch.setattr(hf, "_load", lambda ref: tok)
    monkeypatch.setattr(hf, "_target", lambda ref: (str(tmp_path), "stub"))
    monkeypatch.setattr(hf, "_written", lambda *a, **k: None)
    monkeypatch.setattr(hf, "is_byte_level", lambda t: False)
    monkeypatch.setattr(hf, "_merges_file", lambda *a, **k: None)
    assert hf.export("org/stub")["normalizer"] == "NFKC"
    tok.backend_tokenizer = _StubBackend(None)
    assert hf.export("org/stub")["normalizer"] is None
