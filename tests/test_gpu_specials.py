"""Special tokens on the GPU (csrc/hutk_special.hip) against tests/specials_ref.py over the CPU oracle: ids, offsets and
status of every document, through the host form, the device form and the Python surface.  Needs a real MI355X."""
import random

import numpy as np
import pytest

import collate_ref as R
import helpers as H
import specials_ref as S

pytestmark = pytest.mark.gpu

E_VALUE, E_ARG, E_UNSUPPORTED, E_CAPACITY, E_WORD_TOO_LARGE = 2, 4, 6, 7, 9
EOT = "<|endoftext|>"
VG_MARKERS = {EOT: 50256, "<|im_start|>": 50257, "<|im_end|>": 50258, "<tool_call>": 60000}
VL_MARKERS = {"<s>": 1, "</s>": 2, "<|eot_id|>": 32000, "<|python_tag|>": 32001}
RESERVED = {"<|reserved_special_token_%d|>" % k: 128002 + k for k in range(256)}

_pairs = {}


def _pair(oracle_mod, name, merges=False):
    """-> (GPU context, oracle) of a shipped vocabulary, made once per module."""
    key = (name, merges)
    if key not in _pairs:
        from hutoken_amd import _capi, data
        vp, sp, kw = data.vocab_files(name)
        mp = data.merges_file(name) if merges else None
        ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0, merges_path=mp)
        orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"], merges_path=mp)
        _pairs[key] = (ctx, orc)
    return _pairs[key]


def _raw(specials):
    return {k.encode("utf-8"): v for k, v in specials.items()}


def _pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    if docs:
        np.cumsum([len(x) for x in docs], out=offs[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), offs


def _device(ctx, d, o, ids_cap=None, raw=False):
    """hutk_encode_special_batch_device on a stream of its own -> (ids, out_offsets, status, err) as numpy, or with
    raw=True (return code, the four device tensors)."""
    import torch
    from hutoken_amd import _capi
    dev = torch.device("cuda", 0)
    n = len(o) - 1
    nb = int(o[-1])
    cap = ctx.special_ids_capacity(nb, n) if ids_cap is None else ids_cap
    db = torch.from_numpy(np.array(d, dtype=np.uint8)).to(dev)
    do = torch.from_numpy(np.asarray(o, dtype=np.int64)).to(dev)
    ids = torch.full((max(cap, 1),), -7, dtype=torch.int32, device=dev)
    oo = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    st = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    err = torch.full((1,), -7, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    rc = _capi.load().hutk_encode_special_batch_device(ctx.handle, db.data_ptr() or None, do.data_ptr(), n, nb,
                                                       ids.data_ptr(), cap, oo.data_ptr(), st.data_ptr(),
                                                       err.data_ptr(), side.cuda_stream)
    side.synchronize()
    if raw:
        return rc, ids, oo, st, err
    assert rc == 0, _capi.last_error()
    oo = oo.cpu().numpy()
    return ids.cpu().numpy()[:int(oo[n])], oo, st.cpu().numpy()[:n], int(err.item())


def _check(ctx, orc, docs, specials, tag, min_matches=1, status=False):
    """Host form and device form against the restatement: ids, offsets, status, the number of matches."""
    d, o = _pack(docs)
    ctx.set_special_tokens(sorted(_raw(specials).items()))
    want_ids, want_oo, want_st, matches = S.encode(orc, d, o, _raw(specials))
    assert matches >= min_matches, (tag, matches)
    assert bool(want_st.any()) == status, tag
    ids, oo, st, rc = ctx.encode_special_packed(d, o)
    print("%s: %d docs, %d bytes, %d matches, %d ids, rc %d" % (tag, len(docs), len(d), matches, len(want_ids), rc))
    assert rc == (E_WORD_TOO_LARGE if status else 0), tag
    assert ctx.special_last_matches == matches, tag
    assert np.array_equal(oo, want_oo), (tag, "host offsets")
    assert np.array_equal(ids, want_ids), (tag, "host ids")
    assert np.array_equal(st, want_st), (tag, "host status")
    ids, oo, st, err = _device(ctx, d, o)
    assert err == (E_WORD_TOO_LARGE if status else 0), tag
    assert ctx.special_last_matches == matches, tag
    assert np.array_equal(oo, want_oo), (tag, "device offsets")
    assert np.array_equal(ids, want_ids), (tag, "device ids")
    assert np.array_equal(st, want_st), (tag, "device status")
    return want_ids, want_oo


def _with_markers(rng, markers, n):
    """n random_text documents with markers at random character positions, and the cases that need a place of their own."""
    names = list(markers)
    docs = []
    for _ in range(n):
        t = H.random_text(rng)
        for _ in range(rng.choice([0, 0, 1, 1, 2, 3])):
            at = rng.randint(0, len(t))
            t = t[:at] + rng.choice(names) + t[at:]
        docs.append(t)
    m = names[0]
    docs += [m + "starts", "ends" + m, m + names[1], m + m + m, m, "", "", m + " a space follows", " " + m + " x",
             "a" + m + " b" + names[1] + "  c", m[:-1], m[1:], "x" + m[:-1] + " " + m]
    rng.shuffle(docs)
    return docs


@pytest.mark.parametrize("name,merges,markers", [("VG", False, VG_MARKERS), ("VL", False, VL_MARKERS), ("VG", True, VG_MARKERS)])
def test_parity(oracle_mod, name, merges, markers):
    import hutoken_amd
    from hutoken_amd import data
    ctx, orc = _pair(oracle_mod, name, merges)
    rng = random.Random(41 + merges)
    texts = _with_markers(rng, markers, 200)
    docs = [t.encode("utf-8") for t in texts]
    want_ids, want_oo = _check(ctx, orc, docs, markers, "%s%s parity" % (name, " merges" if merges else ""), min_matches=150)
    if name == "VL":
        assert (want_ids == -1).any()  # unknown units are compared like any other id
    # the Python surface, on the module's own context
    vp, sp, kw = data.vocab_files(name)
    hutoken_amd.initialize(vp, sp, prefix=kw["prefix"], is_byte_encoder=kw["is_byte_encoder"], device=0,
                           merges_file_path=data.merges_file(name) if merges else None)
    assert hutoken_amd.context().special_token_count == 0  # a new initialize() starts without specials
    hutoken_amd.set_special_tokens(markers)
    want = [want_ids[int(want_oo[i]):int(want_oo[i + 1])].tolist() for i in range(len(docs))]
    assert hutoken_amd.batch_encode_special(texts) == want
    for i in range(0, len(texts), 23):
        assert hutoken_amd.encode_special(texts[i]) == want[i], texts[i]
    if name == "VG":
        got = hutoken_amd.encode_special("a" + EOT + "b")
        assert got.count(50256) == 1 and len(got) == 3
        assert hutoken_amd.decode(got) == "a" + EOT + "b"
        plain = hutoken_amd.encode("a" + EOT + "b")  # the plain encode never looks at the set
        assert 50256 not in plain and plain == orc.encode("a" + EOT + "b")
    hutoken_amd.set_special_tokens(None)
    assert hutoken_amd.context().special_token_count == 0


def scan_boundaries_case():
    """-> (documents, the marker set, markers inside the first document): a 29-byte marker every T + 1 bytes of a document
    of 40 T bytes, and markers split over two documents.  (tests/test_gpu_ptiles_edges.py runs it again.)"""
    from hutoken_amd import _capi
    T = _capi.load().hutk_debug_special_tile_bytes()
    m = b"<|reserved_special_token_12|>"
    assert len(m) == 29
    rng = random.Random(2)
    filler = bytearray()
    while len(filler) < 40 * T:
        filler += H.random_text(rng, max_words=40, exotic=0.0).encode("utf-8") + b" "
    big = bytearray(filler[:40 * T])
    n_in = 0
    for at in range(0, len(big) - len(m), T + 1):  # the first one at byte 0
        big[at:at + len(m)] = m
        n_in += 1
    assert n_in >= 39
    tail = b"the batch ends with " + m
    docs = [bytes(big),
            b"split " + m[:28], m[28:] + b" over two documents",  # the last byte would lie in the next document
            b"again " + m[:13], m[13:] + b" in the middle",
            m[:1], m[1:],
            tail]
    d, o = _pack(docs)
    assert bytes(d[-29:]) == m  # a marker ends at the last byte of the batch
    return docs, {m.decode(): 128014}, n_in


def test_scan_boundaries(oracle_mod):
    """A 29-byte marker every T + 1 bytes of a document of 40 T bytes: every alignment across a workgroup's boundary."""
    ctx, orc = _pair(oracle_mod, "VG")
    docs, specials, n_in = scan_boundaries_case()
    _check(ctx, orc, docs, specials, "scan boundaries", min_matches=n_in + 1)
    assert ctx.special_last_matches == n_in + 1  # none of the split ones


def test_overlap_rules(oracle_mod):
    from hutoken_amd import _capi
    ctx, orc = _pair(oracle_mod, "VG")
    T = _capi.load().hutk_debug_special_tile_bytes()
    runs = [b"a" * k for k in range(1, 10)] + [b"b" + b"a" * 5 + b" " + b"a" * 4]
    _check(ctx, orc, runs, {"aa": 7}, "aa on short runs", min_matches=16)
    _check(ctx, orc, [b"x", b"a" * (2 * T + 1), b"aa"], {"aa": 7}, "aa: a chain across workgroups", min_matches=T + 1)
    _check(ctx, orc, [b"abc", b"xabcbc", b"bcab", b"ababc", b"bbc"], {"ab": 1, "bc": 2}, "ab | bc", min_matches=6)
    two = {"<|a|>": 900001, "<|a|><|b": 900002}
    _check(ctx, orc, [b"<|a|><|b|>", b"<|a|><|c|>", b"<|a|><|", b"<|b <|a|>", b"<|a|><|b"], two, "a prefix of another",
           min_matches=5)
    rng = random.Random(8)
    docs = []
    for _ in range(60):
        t = H.random_text(rng)
        for _ in range(rng.randint(0, 3)):
            at = rng.randint(0, len(t))
            t = t[:at] + "<|reserved_special_token_%d|>" % rng.randrange(256) + t[at:]
        docs.append(t.encode("utf-8"))
    docs += [b"<|reserved_special_token_256|>", b"<|reserved_special_token_|>", b"<|reserved_special_token_7"]
    _check(ctx, orc, docs, RESERVED, "256 reserved markers", min_matches=60)


def stitch_cases():
    """-> [(documents, tag, least number of matches)], all for the marker set {EOT: 50256}; the first one is the long piece
    between two markers.  (tests/test_gpu_ptiles_edges.py runs them again.)"""
    rng = random.Random(3)
    m = EOT.encode()
    long_text = " ".join(H.random_text(rng, max_words=30, exotic=0.1) for _ in range(120)).encode("utf-8")
    return [([b"x", m + long_text + m + b" y", b"z" + m], "a long piece between two markers", 3),
            ([b"before ", m * 5000, b" after"], "5000 markers back to back", 5000),
            ([b"in front " + m] + [b""] * 100_000 + [m + b" behind", m], "100 000 empty documents", 3),
            ([b"", b"a" + m, m + m, b" b", b""], "first and last document empty", 3)]


def test_stitch(oracle_mod):
    ctx, orc = _pair(oracle_mod, "VG")
    for k, (docs, tag, least) in enumerate(stitch_cases()):
        want_ids, _ = _check(ctx, orc, docs, {EOT: 50256}, tag, min_matches=least)
        if k == 0:
            assert len(want_ids) > 2048 + 8


def test_no_op(oracle_mod):
    """Nothing installed, nothing found, no documents, no bytes: the plain encode, and zero matches."""
    import torch

    import hutoken_amd
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, prefix=kw["prefix"], is_byte_encoder=kw["is_byte_encoder"], device=0)
    rng = random.Random(6)
    d, o = _pack([H.random_text(rng).encode("utf-8") for _ in range(300)] + [b"<|endoftext", b"|endoftext|>"])
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    db, do = torch.from_numpy(np.array(d)).to(dev), torch.from_numpy(o).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        want_ids, want_oo = hutoken_amd.encode_packed_device(db, do)
        n = int(want_oo[-1].item())
        for specials in (None, VG_MARKERS):
            hutoken_amd.set_special_tokens(specials)
            ids, oo = hutoken_amd.encode_special_packed_device(db, do)
            assert torch.equal(oo, want_oo) and torch.equal(ids[:n], want_ids[:n]), specials
            assert hutoken_amd.context().special_last_matches == 0
        # no documents; documents without bytes
        ids, oo = hutoken_amd.encode_special_packed_device(db[:0], do[:1])
        assert oo.tolist() == [0] and hutoken_amd.context().special_last_matches == 0
        ids, oo = hutoken_amd.encode_special_packed_device(db[:0], torch.zeros(4, dtype=torch.int64, device=dev))
        assert oo.tolist() == [0, 0, 0, 0]
    side.synchronize()
    assert hutoken_amd.batch_encode_special([]) == [] and hutoken_amd.batch_encode_special(["", ""]) == [[], []]
    hutoken_amd.set_special_tokens(None)


def test_cut_piece(oracle_mod):
    """A word over the reference's limit between two markers: that piece ends in front of it, the others are whole."""
    ctx, orc = _pair(oracle_mod, "VG")
    m = EOT.encode()
    docs = [b"one " + m + b"ok " + b"q" * 262_145 + m + b" the rest is intact" + m, b"another document"]
    want_ids, want_oo = _check(ctx, orc, docs, {EOT: 50256}, "cut piece", min_matches=3, status=True)
    first = want_ids[:int(want_oo[1])].tolist()
    assert first.count(50256) == 3
    head, rest = orc.encode("one ") + [50256], [50256] + orc.encode(" the rest is intact") + [50256]
    assert first[:len(head)] == head and first[-len(rest):] == rest
    assert len(first) < len(head) + len(rest) + 4  # of the piece with the word at most "ok" is left


def test_composition_with_collation(oracle_mod):
    """The pair goes through collate_padded and SequencePacker.add as encode_packed_device's does."""
    import torch

    import hutoken_amd
    from hutoken_amd import data
    ctx, orc = _pair(oracle_mod, "VG")
    vp, sp, kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, prefix=kw["prefix"], is_byte_encoder=kw["is_byte_encoder"], device=0)
    hutoken_amd.set_special_tokens(VG_MARKERS)
    rng = random.Random(12)
    docs = [t.encode("utf-8") for t in _with_markers(rng, VG_MARKERS, 150)]
    d, o = _pack(docs)
    ref_ids, ref_oo, _st, _m = S.encode(orc, d, o, _raw(VG_MARKERS))
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    db, do = torch.from_numpy(np.array(d)).to(dev), torch.from_numpy(o).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ids, oo = hutoken_amd.encode_special_packed_device(db, do)
        got = hutoken_amd.collate_padded(ids, oo, 24, eos_id=50256, pad_id=-9, check=True)
        with hutoken_amd.SequencePacker(64, eos_id=50256, pad_id=-9) as p:
            whole = {k: v.cpu().numpy() for k, v in p.add(ids, oo, check=True).items()}
            tail = {k: v.cpu().numpy() for k, v in p.flush().items()}
    side.synchronize()
    want = R.padded(ref_ids, ref_oo, 24, eos_id=50256, pad_id=-9)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    vw, vt = R.packed_vec(ref_ids, ref_oo, 64, eos_id=50256, pad_id=-9)
    assert R.rows_equal(whole, vw) and R.rows_equal(tail, vt)
    hutoken_amd.set_special_tokens(None)


def test_errors(oracle_mod):
    import torch
    from hutoken_amd import _capi, data
    vp, sp, kw = data.vocab_files("VG")
    ctx, _orc = _pair(oracle_mod, "VG")
    ctx.set_special_tokens([(EOT.encode(), 50256)])
    d, o = _pack([b"ab" + EOT.encode(), b"cd"])
    cap = ctx.special_ids_capacity(len(d), 2)
    # ids_cap too small: refused at the call, nothing enqueued (the buffers keep what they held)
    rc, ids, oo, st, err = _device(ctx, d, o, ids_cap=cap - 2, raw=True)
    assert rc == E_CAPACITY and "hutk_special_ids_capacity" in _capi.last_error()
    assert (ids == -7).all() and (oo == -7).all() and (st == -7).all() and int(err.item()) == -7
    # NULL buffers
    L = _capi.load()
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(np.array(d)).to(dev), torch.from_numpy(o).to(dev)
    out = torch.zeros(cap, dtype=torch.int32, device=dev)
    oo = torch.zeros(3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert L.hutk_encode_special_batch_device(ctx.handle, db.data_ptr(), None, 2, len(d), out.data_ptr(), cap,
                                              oo.data_ptr(), None, None, None) == E_ARG
    assert L.hutk_encode_special_batch_device(ctx.handle, None, do.data_ptr(), 2, len(d), out.data_ptr(), cap,
                                              oo.data_ptr(), None, None, None) == E_ARG
    assert L.hutk_encode_special_batch_device(ctx.handle, db.data_ptr(), do.data_ptr(), 2, len(d), out.data_ptr(), cap,
                                              None, None, None, None) == E_ARG
    assert L.hutk_encode_special_batch_device(None, db.data_ptr(), do.data_ptr(), 2, len(d), out.data_ptr(), cap,
                                              oo.data_ptr(), None, None, None) == E_ARG
    # a set the library refuses, on a context with a device
    with pytest.raises(ValueError, match="equal"):
        ctx.set_special_tokens([(b"<a>", 1), (b"<a>", 2)])
    assert ctx.special_token_count == 1
    # a context with a regex pattern: refused at the call, as the spans are
    rx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0)
    rx.set_pattern("[a-z]+")
    rx.set_special_tokens([(EOT.encode(), 50256)])
    rc, ids, _oo, _st, _err = _device(rx, d, o, raw=True)
    assert rc == E_UNSUPPORTED and (ids == -7).all()
    with pytest.raises(ValueError, match="regex"):
        rx.encode_special_packed(d, o)
    rx.close()
