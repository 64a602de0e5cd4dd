"""The split presets gpt2, cl100k and qwen2 on the GPU (csrc/hutk_presplit.hip): the word starts of
pretokenize_packed_device against the sequential restatement (presplit_ref.py), and the ids of every encoder of a
context with a preset against the oracle's ids of the restatement's words, each encoded as a document of its own.  Needs
a real MI355X."""
import functools
import importlib
import json
import locale
import os

import numpy as np
import pytest

import helpers as H
import presplit_cases as PC
import presplit_ref as R
import specials_ref as SR

pytestmark = pytest.mark.gpu

WHOLE = "(.|\n)+"  # the whole-document pattern of test_regex_path.py: the oracle then encodes a document as ONE word


@functools.lru_cache(maxsize=None)
def want_starts(doc, preset):
    return tuple(R.word_starts(doc, preset))


def gpu_starts(docs, preset, shift=0):
    """Word starts per document (relative to it) of one batch; shift: the text is a view that many bytes into a tensor."""
    import torch
    import hutoken_amd as hutoken
    dev = torch.device("cuda", 0)
    data, offs = PC.pack(docs)
    buf = torch.zeros(len(data) + shift + 1, dtype=torch.uint8, device=dev)
    d_bytes = buf[shift:shift + len(data)]
    if data:
        d_bytes.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    d_offs = torch.tensor(offs, dtype=torch.int64, device=dev)
    starts, so = hutoken.pretokenize_packed_device(d_bytes, d_offs, preset)
    starts, so = starts.tolist(), so.tolist()
    assert so[0] == 0 and so[-1] == len(starts) and len(so) == len(docs) + 1
    return [[p - offs[i] for p in starts[so[i]:so[i + 1]]] for i in range(len(docs))]


def check_batch(docs, preset, shift=0):
    got = gpu_starts(docs, preset, shift)
    for i, d in enumerate(docs):
        assert got[i] == list(want_starts(d, preset)), (preset, i, d[:80])


def g13_docs(preset):
    with open(os.path.join(H.GOLDEN_DIR, "g13_presplit.json"), encoding="utf-8") as f:
        return [t.encode("utf-8") for t, _ends in json.load(f)["presets"][preset]]


@pytest.mark.parametrize("preset", R.PRESETS)
def test_word_starts_on_the_golden_texts_and_ill_formed_bytes(preset):
    check_batch(g13_docs(preset), preset)
    check_batch(PC.ill_formed(400, 21) + PC.ILL_FORMED, preset)
    import hutoken_amd as hutoken
    texts = [t.decode() for t in g13_docs(preset)[:40]] + ["", "a", "\udc80x"]
    assert hutoken.pretokenize(texts, preset) == [R.words(t, preset) for t in texts]
    assert hutoken.pretokenize(texts[:5], "llama3") == hutoken.pretokenize(texts[:5], "cl100k")


@pytest.mark.parametrize("preset", R.PRESETS)
def test_carries_over_the_real_chunk_edges(preset):
    from hutoken_amd import _capi
    chunk = _capi.presplit_chunk_bytes()
    assert chunk == 4096
    for t in PC.carry_cases(chunk):  # laid out from byte 0: a batch each
        check_batch([t.encode("utf-8")], preset)


@pytest.mark.parametrize("preset", R.PRESETS)
def test_slice_and_bitmap_word_edges(preset):
    from hutoken_amd import _capi
    chunk = _capi.presplit_chunk_bytes()
    for edge in (64, chunk):
        check_batch([t.encode("utf-8") for t in PC.edge_cases(edge)], preset)  # as documents: every offset mod 32 occurs
    for item in PC.EDGE_ITEMS[:5]:  # ... and from byte 0: a four-byte character, contractions and a space prefix on every edge
        for back in range(36):
            check_batch([("q" * (chunk - back) + item + "z9").encode("utf-8")], preset)


@pytest.mark.parametrize("preset", R.PRESETS)
def test_empty_batches_empty_and_one_byte_documents_and_document_edges(preset):
    assert gpu_starts([], preset) == []
    assert gpu_starts([b"", b"", b""], preset) == [[], [], []]
    check_batch([b"", b"abc def", b"", b"", b"12345", b""], preset)
    check_batch([bytes([b]) for b in b"a' s1\n\t!\x80\xe4"] + [b""] + [bytes([b]) for b in b"'ll"], preset)
    # a document boundary inside what would be one word: two document starts
    check_batch([b"a", b"'s", b"12", b"34", b" ", b"x", b"\n", b"\n", b"!", b"\n\n", b"wor", b"d", b"\xe4\xb8", b"\xad"], preset)
    two = [0, 1] if preset == "qwen2" else [0]
    assert gpu_starts([b"a", b"'s", b"12", b"34"], preset) == [[0], [0], two, two]


@pytest.mark.parametrize("preset", R.PRESETS)
def test_views_at_every_byte_offset(preset):
    docs = [t.encode("utf-8") for t in PC.seeded_texts(40, 31)] + [b"", b"x's 1234 \n\n  y"]
    for shift in range(1, 16):
        check_batch(docs, preset, shift)


def test_offsets_that_do_not_describe_the_bytes_are_refused():
    import torch
    import hutoken_amd as hutoken
    dev = torch.device("cuda", 0)
    d_bytes = torch.full((100,), 97, dtype=torch.uint8, device=dev)
    for offs in ([0, 50, 40, 100], [1, 100], [0, 99], [0, 101], [0, -1, 100]):
        with pytest.raises(ValueError, match="offsets"):
            hutoken.pretokenize_packed_device(d_bytes, torch.tensor(offs, dtype=torch.int64, device=dev), "gpt2")
        before = torch.full((100 // 32 + 40,), 0x55555555, dtype=torch.int32, device=dev)
        bits = hutoken.pretokenize_packed_device(d_bytes, torch.tensor(offs, dtype=torch.int64, device=dev), "cl100k", return_bits=True)
        assert bits.shape == before.shape  # (enqueued only; nothing to compare: the bitmap is left unwritten)
    with pytest.raises(ValueError):
        hutoken.pretokenize_packed_device(d_bytes, torch.tensor([0, 100], dtype=torch.int64, device=dev), "o200k")
    bits = hutoken.pretokenize_packed_device(d_bytes, torch.tensor([0, 100], dtype=torch.int64, device=dev), "gpt2", return_bits=True)
    assert bits.tolist() == [1, 0, 0, 1 << 4] + [0] * 39  # one word, the bit at n_bytes, zero padding


# ---- ids ----
def id_texts():
    texts = [t.replace("\0", "?") for t in PC.seeded_texts(300, 41, 20, 200)]
    return texts + ["", " ", "a", "'s", "x's", "1234567", "  \n\n  a", "!\n\nb", "we'll've  \t done", "日本語のテキスト 123", "a" * 300, " " * 70 + "b"]


@functools.lru_cache(maxsize=None)
def expected_ids(preset, merges, texts=None):
    """Per text, the oracle's ids of the restatement's words, each as a document of its own, concatenated."""
    from hutoken_amd import data
    from oracle import oracle as O
    texts = id_texts() if texts is None else list(texts)
    vp, sp, kw = data.vocab_files("VG")
    orc = O.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"], merges_path=data.merges_file("VG") if merges else None, pattern=WHOLE)
    words = [[w.encode("utf-8") for w in R.words(t, preset)] for t in texts]
    flat = [w for ws in words for w in ws]
    d, o = O.pack(flat) if flat else (np.zeros(0, np.uint8), np.zeros(1, np.int64))
    ids, oo, _st = orc.encode_packed(d, o, 8)
    out, k = [], 0
    for ws in words:
        out.append(ids[oo[k]:oo[k + len(ws)]].tolist())
        k += len(ws)
    orc.close()
    return out


@pytest.fixture(scope="module")
def lc_ctype():
    with open(os.path.join(H.GOLDEN_DIR, "g9_regex_path.json")) as f:
        want = json.load(f)["lc_ctype"]
    if locale.setlocale(locale.LC_CTYPE, None) != want:
        pytest.skip("POSIX regex matching depends on LC_CTYPE; the whole-document pattern was checked under " + want)


def init(preset, merges):
    import hutoken_amd as hutoken
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files("VG")
    hutoken.initialize(vp, sp, is_byte_encoder=True, pretokenizer=preset, merges_file_path=data.merges_file("VG") if merges else None)
    assert hutoken.context().pretokenizer == R.PRESETS.index(R.ALIASES.get(preset, preset))
    return hutoken


@pytest.mark.parametrize("merges", [False, True])
@pytest.mark.parametrize("preset", R.PRESETS)
def test_ids_through_every_encoder(lc_ctype, preset, merges):
    import torch
    from oracle import oracle as O
    hutoken = init(preset, merges)
    texts, want = id_texts(), expected_ids(preset, merges)
    dev = torch.device("cuda", 0)
    data, offs = O.pack(texts)
    d_bytes, d_offs = torch.from_numpy(np.array(data, copy=True)).to(dev), torch.from_numpy(np.array(offs, copy=True)).to(dev)
    ids, oo = hutoken.encode_packed_device(d_bytes, d_offs, check=True)
    oo = oo.tolist()
    ids = ids[:oo[-1]].tolist()
    got = [ids[oo[i]:oo[i + 1]] for i in range(len(texts))]
    bad = [i for i in range(len(texts)) if got[i] != want[i]]
    assert not bad, (bad[:5], texts[bad[0]], got[bad[0]][:20], want[bad[0]][:20])
    # check=False: enqueued on the current stream, tensors back, nothing waited for
    ids2, oo2 = hutoken.encode_packed_device(d_bytes, d_offs, check=False)
    assert ids2.is_cuda and oo2.is_cuda and oo2.tolist() == oo and ids2[:oo[-1]].tolist() == ids
    assert hutoken.batch_encode(texts, 2) == want
    for i in (0, 1, 2, len(texts) - 3, len(texts) - 2):
        if texts[i]:
            assert hutoken.encode(texts[i]) == want[i], texts[i]
    # the host path in chunks: the batch repeated until the pipelined path takes it and cuts it several times
    ctx = hutoken.context()
    reps = (49 << 20) // len(data) + 1
    big = np.tile(np.asarray(data), reps)
    big_offs = (np.asarray(offs[:-1])[None, :] + (np.arange(reps) * len(data))[:, None]).reshape(-1)
    big_offs = np.append(big_offs, reps * len(data)).astype(np.int64)
    ids_h, oo_h, _st, rc = ctx.encode_packed(big, big_offs)
    assert rc == 0
    flat = np.array([x for row in want for x in row], dtype=np.int32)
    assert oo_h[-1] == reps * len(flat) and np.array_equal(ids_h[:oo_h[-1]].reshape(reps, -1), np.tile(flat, (reps, 1)))
    lens = np.array([len(r) for r in want], dtype=np.int64)
    assert np.array_equal(np.diff(oo_h).reshape(reps, -1), np.tile(lens, (reps, 1)))


@pytest.mark.parametrize("preset", R.PRESETS)
def test_special_tokens_with_a_preset(lc_ctype, preset):
    hutoken = init(preset, False)
    specials = {"<|endoftext|>": 50256, "<|sep|>": 60000, "<x>": 60001}
    hutoken.set_special_tokens(specials)
    raw = {k.encode(): v for k, v in specials.items()}
    texts = ["hello<|endoftext|>world", "<|sep|> we'll<x>'ll see", "12<x>3456<x>7 89", "a <|sep|>\n\n<|sep|>  b", "<x>", "no marker 123456",
             " <|endoftext|> ", "x<x>'s<x>s", "tab\t<|sep|>\tb!!<x>\n", "<|endoftext|><|endoftext|>", "1234<|sep|>5678901"]
    texts += [t.replace("\0", "?")[:60] + "<x>" + t[60:].replace("\0", "?") for t in PC.seeded_texts(40, 43, 70, 200)]
    plan = [SR.pieces(t.encode("utf-8"), raw) for t in texts]
    pieces = tuple(sorted({p.decode("utf-8") for pl in plan for p in pl if isinstance(p, bytes)}))
    ids_of = dict(zip(pieces, expected_ids(preset, False, pieces)))
    want = [[x for p in pl for x in (ids_of[p.decode("utf-8")] if isinstance(p, bytes) else [p])] for pl in plan]
    assert hutoken.batch_encode_special(texts) == want
    assert hutoken.encode_special(texts[2]) == want[2]
    hutoken.set_special_tokens(None)


@pytest.mark.parametrize("preset", R.PRESETS)
def test_spans_with_a_preset(lc_ctype, preset):
    hutoken = init(preset, False)
    texts = [t for t in id_texts() if t][:120]
    want = expected_ids(preset, False)
    ids_b, spans_b = hutoken.batch_encode_with_offsets(texts, unit="byte")
    for t, ids, spans in zip(texts, ids_b, spans_b):
        raw = t.encode("utf-8")
        assert ids == want[id_texts().index(t)]
        assert [a for a, _b in spans] == [0] + [b for _a, b in spans[:-1]] and spans[-1][1] == len(raw)  # they tile the document
        for i, (a, b) in zip(ids, spans):
            try:
                piece = raw[a:b].decode("utf-8")
            except UnicodeDecodeError:
                continue  # (a token that is part of a character has no text of its own)
            assert hutoken.decode([i]) == piece
    ascii_texts = [t for t in texts if t.isascii()] + ["we'll see 12345 things!\n\n  ok", "x's"]
    ids_c, spans_c = hutoken.batch_encode_with_offsets(ascii_texts, unit="char")
    for t, ids, spans in zip(ascii_texts, ids_c, spans_c):
        assert [a for a, _b in spans] == [0] + [b for _a, b in spans[:-1]] and spans[-1][1] == len(t)
        assert [hutoken.decode([i]) for i in ids] == [t[a:b] for a, b in spans]


def test_a_word_over_the_limit_ends_its_document_under_gpt2():
    """A run of 262145 letters ends its document in front of it, one of 262144 encodes: status and ids as the plain path
    gives for the same words (test_gpu_cut.py, NO_SEAM_DOCS: letters and single spaces split alike under both)."""
    import test_gpu_cut as TC
    from hutoken_amd import _capi, data
    PT = importlib.import_module("hutoken_amd.pretokenize")
    from oracle import oracle as O
    vp, sp, kw = data.vocab_files("VG")
    plain = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    ctx.set_pretokenizer(PT.preset_index("gpt2"), PT.table_blob())
    d, o = O.pack(TC.NO_SEAM_DOCS)
    ids_p, oo_p, st_p, _err = TC.device_form(plain, d, o)
    ids_g, oo_g, st_g, err_g = TC.device_form(ctx, d, o)
    assert st_g.tolist() == st_p.tolist() == TC.NO_SEAM_STATUS and err_g in (0, 9)
    assert np.array_equal(oo_g, oo_p) and np.array_equal(ids_g, ids_p)
    ids_h, oo_h, st_h, rc = ctx.encode_packed(d, o)  # the host entry point
    assert rc == 0 and st_h.tolist() == TC.NO_SEAM_STATUS and np.array_equal(oo_h, oo_p) and np.array_equal(ids_h[:oo_h[-1]], ids_p)
    # the run alone is the word (a newline in front of it is a word of its own): 262145 letters cut, 262144 do not
    head = b"letters over the limit\n"
    docs = [head + b"x" * (TC.LIMIT + 1) + b" dropped", head + b"x" * TC.LIMIT + b" kept", head]
    d, o = O.pack(docs)
    ids, oo, st, err = TC.device_form(ctx, d, o)
    assert st.tolist() == [1, 0, 0] and err in (0, 9)
    assert ids[oo[0]:oo[1]].tolist() == ids[oo[2]:oo[3]].tolist()  # what stands in front of the word
    assert oo[2] - oo[1] > oo[1] - oo[0] + 2 and ids[oo[1]:oo[1] + oo[1] - oo[0]].tolist() == ids[oo[0]:oo[1]].tolist()
    plain.close()
    ctx.close()


def test_refusals(tmp_path):
    from hutoken_amd import _capi, data
    PT = importlib.import_module("hutoken_amd.pretokenize")
    blob = PT.table_blob()
    vp, sp, kw = data.vocab_files("VL")
    with_prefix = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    with pytest.raises(Exception, match="prefix"):
        with_prefix.set_pretokenizer(0, blob)
    with_prefix.close()
    vp, sp, kw = data.vocab_files("VG")
    ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    ctx.set_pattern("[a-z]+")
    with pytest.raises(Exception, match="pattern"):
        ctx.set_pretokenizer(1, blob)
    ctx.set_pattern(None)
    ctx.set_pretokenizer(1, blob)
    assert ctx.pretokenizer == 1
    with pytest.raises(Exception, match="preset"):
        ctx.set_pattern("[a-z]+")
    ctx.set_pretokenizer(None)
    assert ctx.pretokenizer is None
    ctx.close()
    with pytest.raises(Exception, match="tables"):
        _capi.Pretokenizer(blob[:-4], 0)
    import hutoken_amd as hutoken
    hutoken.initialize(vp, sp, is_byte_encoder=True, pretokenizer="qwen2")
    hutoken.set_byte_fallback([i for i in range(256)])
    with pytest.raises(Exception, match="preset"):
        hutoken.batch_encode_fallback(["abc"])
    with pytest.raises(ValueError):
        hutoken.initialize(vp, sp, is_byte_encoder=True, pretokenizer="o200k")
    hutoken.set_pretokenizer(None)
    assert hutoken.context().pretokenizer is None
    hutoken.initialize(vp, sp, is_byte_encoder=True)
