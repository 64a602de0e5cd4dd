"""Shared builders for small vocabularies and adversarial texts (own code, seeded)."""
import contextlib
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hutoken_amd import vocab_files as vf  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
G12_PATH = os.path.join(GOLDEN_DIR, "g12_reference_answers.json.gz")

BLOCK_DOCS = 100_000


def block_hashes(ids, oo, block=BLOCK_DOCS):
    """Per block of `block` documents: id count, sha256 of the ids (int32 LE), sha256 of the block-relative
    offsets (int64 LE).  The unit of tests/golden/g7_full.json."""
    import hashlib

    import numpy as np
    ids = np.asarray(ids)
    oo = np.asarray(oo, dtype=np.int64)
    out = []
    n = len(oo) - 1
    for a in range(0, n, block):
        b = min(a + block, n)
        seg = ids[int(oo[a]):int(oo[b])].astype("<i4", copy=False)
        rel = (oo[a:b + 1] - oo[a]).astype("<i8", copy=False)
        out.append({"n_ids": int(oo[b] - oo[a]), "ids_sha256": hashlib.sha256(seg.tobytes()).hexdigest(),
                    "offsets_sha256": hashlib.sha256(rel.tobytes()).hexdigest()})
    return out


HU = "áéíóöőúüűÁÉÍÓÖŐÚÜŰ"
CJK = "漢字仮名交じり文中文測試"
EMOJI = "😂🙂🚀"
ODD = " €—…«»"


def random_byte_vocab(seed, n_merges=300, proper=True, dup_ids=False, neg_ids=False, max_len=12):
    """GPT-2-shaped byte-level vocabulary: 256 byte tokens then `n_merges`
    tokens that are concatenations of two earlier tokens (proper=True) or
    arbitrary short byte strings with shuffled ids (proper=False).
    Returns (entries [(visible-bytes, id)], special mapping)."""
    rng = random.Random(seed)
    t = vf.bytes_to_unicode()
    order = vf.byte_token_order()
    raw_tokens = [bytes([b]) for b in order]
    alphabet = (b"etaoinshrdlucmfwypvbgkqjxz" * 3 + b" " * 6 + b"ETAOIN0123456789.,!?\n\t"
                + "áéőű漢😂".encode("utf-8"))
    seen = set(raw_tokens)
    while len(raw_tokens) < 256 + n_merges:
        if proper:
            a = raw_tokens[rng.randrange(len(raw_tokens))]
            b = rng.choice(raw_tokens)
            if rng.random() < 0.7:
                a = bytes([rng.choice(alphabet)]) if rng.random() < 0.5 else a
            tok = a + b
        else:
            tok = bytes(rng.choice(alphabet) for _ in range(rng.randint(2, 5)))
        if tok in seen or len(tok) > max_len:
            continue
        seen.add(tok)
        raw_tokens.append(tok)
    ids = list(range(len(raw_tokens)))
    if not proper:
        tail = ids[256:]
        rng.shuffle(tail)
        ids[256:] = tail
    if dup_ids:
        for _ in range(n_merges // 10):
            i = rng.randrange(256, len(ids))
            ids[i] = ids[rng.randrange(256, len(ids))]
    if neg_ids:
        for _ in range(n_merges // 20):
            ids[rng.randrange(256, len(ids))] = rng.choice([-1, -2, -7])
    entries = [(vf.encode_visible(tok, t), i) for tok, i in zip(raw_tokens, ids)]
    return entries, vf.gpt2_special_mapping()


def random_char_vocab(seed, n_merges=300, drop_chars="", max_len=10):
    """SentencePiece/Llama-shaped vocabulary (is_byte_encoder=False,
    prefix U+2581): single characters, byte-fallback literals <0xHH>, and
    merges of earlier tokens.  Characters in `drop_chars` are left out so that
    they encode to -1 yet can still appear inside longer tokens."""
    rng = random.Random(seed)
    chars = list("▁etaoinshrdlucmfwypvbgkqjxzETAOIN0123456789.,!?-") + list(HU) + list(CJK[:6])
    toks = ["<0x%02X>" % b for b in range(256)]
    toks += [c for c in chars if c not in drop_chars]
    base = list(chars)
    seen = set(toks)
    while len(toks) < 256 + len(chars) + n_merges:
        a = rng.choice(base if rng.random() < 0.5 else toks[256:])
        b = rng.choice(base if rng.random() < 0.5 else toks[256:])
        tok = a + b
        if tok in seen or len(tok) > max_len:
            continue
        seen.add(tok)
        toks.append(tok)
    entries = [(tk.encode("utf-8"), i) for i, tk in enumerate(toks)]
    return entries, vf.llama_special_mapping()


def random_merges_text(entries, seed, keep=0.85, noise=True):
    """A merges.txt for the id-keyed merge path (reference lib.c:573-663): every split of a vocabulary key
    into two vocabulary keys is a possible rule; a random subset in random order (so rank != id order), plus
    the lines the loader has to cope with: comments, lines without a space, runs of spaces, rules with
    unknown tokens (skipped, take no rank), a repeated pair (the later line and rank win), CRLF endings."""
    rng = random.Random(seed)
    keys = {}
    for k, i in entries:
        keys[k] = i
    rules = []
    for k in keys:
        try:
            txt = k.decode("utf-8")
        except UnicodeDecodeError:
            continue
        for cut in range(1, len(txt)):
            a, b = txt[:cut].encode("utf-8"), txt[cut:].encode("utf-8")
            if a in keys and b in keys and b" " not in k:
                rules.append((a, b))
    rng.shuffle(rules)
    rules = rules[: int(len(rules) * keep)]
    lines = ["#version: 0.2"]
    for a, b in rules:
        sep = " " if not noise or rng.random() < 0.9 else "   "
        end = "" if not noise or rng.random() < 0.9 else "\r"
        lines.append(a.decode("utf-8") + sep + b.decode("utf-8") + end)
        if noise:
            r = rng.random()
            if r < 0.03:
                lines.append("# a comment with a space")
            elif r < 0.06:
                lines.append("nospacehere")
            elif r < 0.09:
                lines.append("zzqx notinvocabq")
            elif r < 0.12 and len(lines) > 5:
                lines.append(rng.choice(lines[1:]))  # an earlier line again
            elif r < 0.13:
                lines.append(a.decode("utf-8") + " ")  # right half missing
    return "\n".join(lines) + "\n"


def write_merges(tmpdir, name, text):
    mp = os.path.join(str(tmpdir), name + "_merges.txt")
    with open(mp, "w", encoding="utf-8", newline="") as f:
        f.write(text)
    return mp


def write_vocab(tmpdir, name, entries, special):
    vp = os.path.join(str(tmpdir), name + "_vocab.txt")
    sp = os.path.join(str(tmpdir), name + "_special.txt")
    vf.write_vocab_file(vp, entries)
    vf.write_special_file(sp, special)
    return vp, sp


def random_text(rng, max_words=12, exotic=0.3):
    """Valid-UTF-8 text that exercises every splitter rule."""
    parts = []
    for _ in range(rng.randint(0, max_words)):
        r = rng.random()
        if r < 0.45:
            w = "".join(rng.choice("etaoinshrdlucmfwypvbgkqjxz") for _ in range(rng.randint(1, 9)))
            if rng.random() < 0.15:
                w = w.capitalize()
        elif r < 0.55:
            w = "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 5)))
        elif r < 0.65:
            w = "".join(rng.choice(".,!?-()\"'") for _ in range(rng.randint(1, 3)))
        elif r < 0.65 + exotic * 0.4:
            w = "".join(rng.choice("aeiou" + HU) for _ in range(rng.randint(1, 7)))
        elif r < 0.65 + exotic * 0.7:
            w = "".join(rng.choice(CJK) for _ in range(rng.randint(1, 5)))
        elif r < 0.65 + exotic * 0.85:
            w = rng.choice(EMOJI) * rng.randint(1, 2)
        else:
            w = rng.choice(ODD)
        sep = rng.choice([" "] * 12 + ["  ", "   ", "\n", "\t", "\r\n", "", "", ", ", ". "])
        parts.append(w + sep)
    s = "".join(parts)
    if rng.random() < 0.2:
        s = " " + s
    return s


def random_bytes_text(rng, n):
    """Arbitrary bytes without 0x00: truncated and invalid UTF-8 included."""
    pool = [b"a", b"b", b" ", b"  ", b"1", b".", b"\t", b"\xc3\xa9", b"\xc5\x91", b"\xe6\xbc\xa2",
            b"\xf0\x9f\x98\x82", b"\xc3", b"\xe6\xbc", b"\xf0\x9f", b"\x80", b"\xbf", b"\xff",
            b"\xc0\xa0", b"\xc1\xa1", b"\xc0\x80", b"\xc2\xa0", b"\xc2\x85", b"\xe0\x80\x80", b"\n"]
    out = b"".join(rng.choice(pool) for _ in range(n))
    return out


_g12 = None


def g12():
    """tests/golden/g12_reference_answers.json.gz: the compiled reference's answers (tools/make_golden_g12.py)."""
    global _g12
    if _g12 is None:
        import gzip
        import json
        with gzip.open(G12_PATH, "rt", encoding="ascii") as f:
            _g12 = json.load(f)
    return _g12


def giant_word_docs():
    """-> (documents with words of 1100 .. 30000 bytes that really merge, ONE document "q " + a word of 262143 bytes, the
    reference's limit): tests/test_gpu_parity.py::test_giant_words, seeded."""
    rng = random.Random(29)
    pieces = [b"international", b"szolg", "árvíztűrő".encode(), b"xq", b"the", b"ation"]

    def blob(n):
        parts, size = [], 0
        while size < n:
            parts.append(rng.choice(pieces))
            size += len(parts[-1])
        return b"".join(parts)[:n]
    docs = [b"a " + blob(1100) + b" b", blob(5000), b"x " + blob(30000), blob(2047) + b" " + blob(1025)]
    return docs, b"q " + blob(262143)


LONG_BYTE_RUNS = list(range(13, 41)) + [48, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300]
LONG_CHAR_RUNS = [5, 11, 12, 13, 20, 21, 22, 40, 64, 100]


def long_token_byte_vocab(seed):
    """random_byte_vocab(seed, n_merges=300) plus run tokens of 13 .. 300 characters ("-", " ", "é" and "abab.." runs;
    an "é" run is twice as many bytes): what the decode direction meets in a real GPT-2 vocabulary and the small
    builders never make.  -> (entries, special mapping, raw token bytes by id); the added ids are 556 and up."""
    entries, special = random_byte_vocab(seed, n_merges=300)
    t = vf.bytes_to_unicode()
    back = {c: b for b, c in t.items()}
    raw = [bytes(back[c] for c in key.decode("utf-8")) for key, _i in entries]
    seen = set(raw)
    for k in LONG_BYTE_RUNS:
        for tok in (b"-" * k, b" " * k, ("é" * k).encode("utf-8"), (b"ab" * k)[:k]):
            assert tok not in seen
            seen.add(tok)
            entries.append((vf.encode_visible(tok, t), len(raw)))
            raw.append(tok)
    return entries, special, raw


def long_token_char_vocab(seed):
    """random_char_vocab(seed, n_merges=300) plus run tokens of 5 .. 100 characters (prefix runs, "a" runs, three-byte
    "漢" runs, the prefix and an "e" run).  -> (entries, special mapping, token strings by id)."""
    entries, special = random_char_vocab(seed, n_merges=300)
    toks = [key.decode("utf-8") for key, _i in entries]
    seen = set(toks)
    for k in LONG_CHAR_RUNS:
        for tok in ("▁" * k, "a" * k, "漢" * k, "▁" + "e" * k):
            if tok in seen:  # (a five-character run the merges happened to make already)
                continue
            seen.add(tok)
            entries.append((tok.encode("utf-8"), len(toks)))
            toks.append(tok)
    return entries, special, toks


def compare(ctx, orc, docs, tag="", encode=None, want_rc=0):
    """docs: list[bytes] without 0x00.  Every id, output offset and per-document status of the GPU against the CPU oracle,
    and the return code: bit-exact.  encode: (data, offsets) -> (ids, out_offsets, status, rc), by default the context's
    host form (ctx.encode_packed); tests/test_gpu_ptiles_edges.py passes the device form, which no small-batch short cut
    takes.  want_rc: 0, or the note E_WORD_TOO_LARGE (9) for a batch in which the oracle cuts a document."""
    import numpy as np
    from oracle import oracle as O
    data, offs = O.pack(docs)
    ids_o, oo_o, st_o = orc.encode_packed(data, offs, num_threads=4)
    ids_g, oo_g, st_g, rc = (encode or ctx.encode_packed)(data, offs)
    assert rc == want_rc, f"{tag}: rc={rc}"
    if not np.array_equal(oo_o, oo_g):
        bad = int(np.nonzero(oo_o != oo_g)[0][0])
        d = max(bad - 1, 0)
        raise AssertionError(
            f"{tag}: out_offsets differ first at {bad}; doc {d}={docs[d][:200]!r}\n"
            f" oracle={ids_o[oo_o[d]:oo_o[d + 1]].tolist()[:200]}\n gpu   ={ids_g[oo_g[d]:oo_g[d + 1]].tolist()[:200]}")
    if not np.array_equal(ids_o, ids_g):
        k = int(np.nonzero(ids_o != ids_g)[0][0])
        d = int(np.searchsorted(oo_o, k, side="right") - 1)
        raise AssertionError(
            f"{tag}: ids differ first at {k} (doc {d}={docs[d][:200]!r})\n"
            f" oracle={ids_o[oo_o[d]:oo_o[d + 1]].tolist()[:200]}\n gpu   ={ids_g[oo_g[d]:oo_g[d + 1]].tolist()[:200]}")
    assert np.array_equal(st_g, st_o), f"{tag}: status"
    if want_rc == 0:
        assert (st_g == 0).all()


# ---- seeded inputs of tests/test_gpu_parity.py that tests/test_gpu_ptiles_edges.py runs through the persistent tile kernel too

def ragged_docs():
    """test_document_boundaries_inside_characters: documents end in the middle of multi-byte sequences and tiles end in the
    middle of words."""
    rng = random.Random(7)
    blob = "".join(random_text(rng, max_words=30) for _ in range(400)).encode("utf-8").replace(b"\0", b"")
    docs, i = [], 0
    while i < len(blob):
        n = rng.choice([0, 1, 2, 3, 5, 17, 64, 300, 2047, 2048, 2049, 5000])
        docs.append(blob[i:i + n])
        i += n
    return docs


def long_word_docs():
    """test_long_words_exception_path: words beyond one lane's capacity, beyond the staged window, and beyond the LDS
    capacity of the exception kernel (1024 units)."""
    rng = random.Random(11)
    docs = []
    for n in [47, 48, 49, 50, 62, 63, 64, 65, 100, 126, 127, 128, 129, 130, 191, 192, 193, 255, 256, 257, 300, 1000, 1023, 1024,
              1025, 1500, 2045, 2046, 2047, 2048, 2049, 3000, 9000]:
        docs.append(bytes(rng.choice(b"etaoinshr") for _ in range(n)))
        docs.append(b"pre " + bytes(rng.choice(b"etaoin") for _ in range(n)) + b" post")
        docs.append(("漢" * (n // 3 + 1)).encode("utf-8"))
    docs.append(b"a" * 5000 + b" " + b"b" * 2100)
    docs.append(b" " * 3000)
    docs.append(b"1" * 2500 + b"x" * 2500)
    return docs


def later_tile_word_docs():
    """test_word_ends_in_later_tiles -> (documents, the seeded word maker that made them): words that end exactly on tile
    limits (multiples of 960 bytes), one to three tiles further on, at a document's end, at the end of the batch, with
    another long word or nothing behind."""
    rng = random.Random(960)

    def word(n):
        return bytes(rng.choice(b"etaoinshrdlu") for _ in range(n))
    docs = []
    for lead in (0, 1, 5, 63, 64, 100, 500, 896, 897, 959, 960, 961, 1000):
        for n in (64, 65, 100, 959 - lead % 960, 960, 961, 1024, 1025, 1919, 1920, 1921, 2880, 3000):
            if n < 64:
                continue
            pre = (word(lead - 1) + b" ") if lead else b""
            docs.append(pre + word(n))                  # the document ends with the word
            docs.append(pre + word(n) + b" x")          # a short word behind
            docs.append(pre + word(n) + b" " + word(n))  # a long one behind
    docs.append(word(70))      # the batch ends with a long word
    return docs, word


def dense_word_docs():
    """test_dense_word_tiles: every byte a word (newlines, stray bytes), and two-byte words back to back (the most
    multi-unit words a tile can start)."""
    return [b"\n" * 5000, b"\xff\x80" * 3000, b"a " * 4000, b" a" * 4000, b"ab" + b"\tab" * 3000,
            b"a1" * 3000, b".a" * 3000 + b"!" * 2000, bytes(range(1, 256)) * 20]


def merge_loop_words(rng, n_words, lo, hi):
    """test_merge_pool_overflow: random letter strings over eight rare letters, so nearly none is a vocabulary key and all
    of them need the merge loop."""
    return b" ".join(bytes(rng.choice(b"qxzjkvwy") for _ in range(rng.randint(lo, hi))) for _ in range(n_words))


# ---- batches through the device entry point (tests/test_gpu_ptiles_edges.py, tests/test_gpu_exc_kinds.py)

E_DEVICE, E_WORD_TOO_LARGE = 5, 9


@contextlib.contextmanager
def env_switches(**kv):
    """Switches for the time of one call, None = unset (HUTK_PTILES is read by every encode, the others when a context is
    made)."""
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_side = None


def side_stream():
    """One stream for the module.  (Not torch's current one: that is the null stream, for which the context takes its own.)"""
    global _side
    if _side is None:
        import torch
        _side = torch.cuda.Stream(torch.device("cuda", 0))
    return _side


class DeviceBatch:
    """A batch on the device; run() encodes it through hutk_encode_batch_device into fresh output buffers.  A device error --
    a HIP failure, or HUTK_E_DEVICE from the kernel's own watchdog -- ends the whole session: nothing more is started on a
    GPU that has faulted or hung."""

    def __init__(self, ctx, data, offs):
        import torch
        self.ctx, self.dev = ctx, torch.device("cuda", 0)
        self.n, self.nb = len(offs) - 1, int(offs[-1])
        self.db = torch.from_numpy(np.array(data[:self.nb], dtype=np.uint8, copy=True)).to(self.dev)
        self.do = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(self.dev)
        self.cap = ctx.ids_capacity(self.nb, self.n)

    def run(self, stream=None):
        import torch
        ids = torch.full((max(self.cap, 1),), -7, dtype=torch.int32, device=self.dev)
        oo = torch.full((self.n + 1,), -7, dtype=torch.int64, device=self.dev)
        st = torch.full((max(self.n, 1),), -7, dtype=torch.int32, device=self.dev)
        err = torch.full((1,), -7, dtype=torch.int32, device=self.dev)
        s = stream if stream is not None else side_stream()
        s.wait_stream(torch.cuda.current_stream(self.dev))  # (the copies and fills above)
        try:
            self.ctx.encode_device(self.db.data_ptr(), self.do.data_ptr(), self.n, self.nb, ids.data_ptr(), self.cap,
                                   oo.data_ptr(), st.data_ptr(), err.data_ptr(), s.cuda_stream)
            s.synchronize()
            e = int(err.item())
        except RuntimeError as ex:
            pytest.exit("device failure, nothing more is run: %s" % ex, returncode=3)
        if e == E_DEVICE:
            pytest.exit("HUTK_E_DEVICE (the kernel's watchdog), nothing more is run", returncode=3)
        oo = oo.cpu().numpy()
        if e not in (0, E_WORD_TOO_LARGE):  # (an error: ids and offsets are not defined)
            return np.zeros(0, dtype=np.int32), oo, st.cpu().numpy()[:self.n], e
        total = int(oo[-1])
        assert 0 <= total <= self.cap, total
        return ids[:total].cpu().numpy(), oo, st.cpu().numpy()[:self.n], e


def device_encoder(ctx, want, twin):
    """-> encode(data, offsets) for H.compare: asserts that hutk_debug_tile_kernel reports `want` for the batch, encodes it
    on the device and, with `twin`, once more through k_tiles on the same buffers: everything the two write must be equal."""
    def encode(data, offs):
        nb = int(offs[-1])
        assert ctx.tile_kernel(nb) == (want if nb else 0), "the batch would not be given the kernel this test is about"
        b = DeviceBatch(ctx, data, offs)
        got = b.run()
        if twin:
            with env_switches(HUTK_PTILES="0"):
                assert ctx.tile_kernel(nb) == 0
                ref = b.run()
            assert got[3] == ref[3], ("error word", got[3], ref[3])
            assert np.array_equal(got[2], ref[2]), "status differs from k_tiles"
            assert np.array_equal(got[1], ref[1]), "out_offsets differ from k_tiles"
            assert np.array_equal(got[0], ref[0]), "ids differ from k_tiles"
        return got
    return encode
