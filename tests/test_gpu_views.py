"""Every device entry point on views off the 16-byte boundary: the element-by-element side of each kernel's alignment
test, which tensors fresh from the caching allocator (aligned to 512 bytes) never reach.

Expected values are the plain references (norm_ref, spans_ref, specials_ref, fallback_ref, collate_ref, the oracle); the
same call on an aligned view is compared as a second assertion.  Every shifted call asserts data_ptr() % 16 != 0 on the
view it means to misalign and the aligned twin asserts == 0, so a shift that moves nothing fails.  Outputs sit in
view_cases.guarded buffers: exactly the output's elements are written.  tests/test_views_cpu.py holds the batches to their
claims without a GPU.  Needs a real MI355X."""
import importlib

import numpy as np
import pytest

import collate_ref as CR
import decode_ref as DR
import fallback_ref as F
import helpers as H
import norm_ref as R
import spans_ref as S
import specials_ref as SR
import view_cases as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G32 = -0x5A5A5A5B  # guard value of the integer outputs
E_ARG, E_UNSUPPORTED = 4, 6
FB_SPECIAL = 1


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def off16(t):
    assert t.data_ptr() % 16 != 0, "the view is on the 16-byte boundary: the shift moved nothing"
    return t


def on16(t):
    assert t.data_ptr() % 16 == 0
    return t


def view(t, shift):
    """the tensor itself (aligned) for shift 0, else a view `shift` elements off the boundary; asserted either way"""
    return on16(t) if shift == 0 else off16(V.shifted(t, shift))


def tdtype(width):
    import torch
    return torch.int32 if width == 4 else torch.int64


def _shipped(oracle_mod, name):
    from hutoken_amd import _capi, data
    vp, sp, kw = data.vocab_files(name)
    return (_capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0),
            oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]), kw["is_byte_encoder"])


# ---- 1. normalisation ---------------------------------------------------------------------------------------------------
def _chunk():
    from hutoken_amd import _capi
    return _capi.norm_chunk_bytes()


_refs = {}


def _reference(name, form, docs):
    if (name, form) not in _refs:
        _refs[name, form] = R.reference(form, docs)
    return _refs[name, form]


def _norm_batches():
    C = _chunk()
    out = [("edges", R.edge_docs(C))]
    out += [("boundary%d" % i, b) for i, b in enumerate(R.boundary_batches(C))]
    out += [("random", R.random_docs()[:3000]), ("fuzz", R.byte_fuzz_docs()[:500]), ("clean", V.clean_docs(C))]
    return out


@pytest.fixture(scope="module")
def normalizer():
    from hutoken_amd import _capi
    tables = importlib.import_module("hutoken_amd.normalize")
    nz = _capi.Normalizer(tables.table_blob(), 0)
    yield nz
    nz.close()


@pytest.mark.parametrize("shift", [1, 3, 8, 15])
def test_normalize_reads_text_off_the_boundary(shift):
    """slice_dirty's byte loop (a.wide false) and, for the clean batch, k_norm_write's copy with src and dst in different
    residues: head = n, the whole chunk byte by byte."""
    import hutoken_amd
    for name, docs in _norm_batches():
        data, offs = R.pack(docs)
        db, do = off16(V.shifted(dev(data.copy()), shift)), dev(offs)
        for form in R.FORMS:
            out, oo, ch = hutoken_amd.normalize_packed_device(db, do, form, copy=True, return_changed=True, check=True)
            rd, ro, rc = _reference(name, form, docs)
            tag = (name, form, shift)
            assert np.array_equal(oo.cpu().numpy(), ro), tag
            assert np.array_equal(ch.cpu().numpy(), rc), tag
            got = out.cpu().numpy()
            assert got.shape == rd.shape and np.array_equal(got, rd), tag
        if name == "clean":
            out, oo, ch = hutoken_amd.normalize_packed_device(db, do, "NFC", return_changed=True)
            assert out is db and oo is do and not ch.any().item()
            aligned = on16(dev(data.copy()))
            twin = hutoken_amd.normalize_packed_device(aligned, do, "NFC", copy=True)[0]
            assert np.array_equal(twin.cpu().numpy(), _reference(name, "NFC", docs)[0])


def norm_capi(nz, fi, d_bytes, d_offs, out_shift):
    """The C ABI: the sizes call, then the write call into guarded(total, out_shift).
    -> (output view, guard check, out_offsets, changed) with everything synchronised"""
    import torch
    n_docs, n_bytes = d_offs.numel() - 1, d_bytes.numel()
    oo = torch.full((n_docs + 1,), -1, dtype=torch.int64, device=DEV)
    ch = torch.full((max(n_docs, 1),), 7, dtype=torch.uint8, device=DEV)
    small = torch.zeros(4, dtype=torch.int64, device=DEV)  # the two totals; the error words of the two calls
    st = torch.cuda.current_stream().cuda_stream
    text = (fi, d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes)
    nz.batch_device(*text, 0, 0, oo.data_ptr(), ch.data_ptr(), small.data_ptr(), small.data_ptr() + 16, st)
    total, _changed, code, _ = small.tolist()
    assert code == 0
    out, check = V.guarded(total, out_shift, torch.uint8, V.GUARD_BYTE)
    nz.batch_device(*text, out.data_ptr(), total, 0, 0, 0, small.data_ptr() + 24, st)
    torch.cuda.synchronize()
    assert int(small[3].item()) == 0
    return out, check, oo.cpu().numpy(), ch.cpu().numpy()[:n_docs]


def _norm_check(nz, form, docs, in_shift, out_shift, tag, ref=None):
    data, offs = R.pack(docs)
    db = view(dev(data.copy()), in_shift)
    out, check, oo, ch = norm_capi(nz, R.FORMS.index(form), db, dev(offs), out_shift)
    if out_shift:
        off16(out)
    rd, ro, rc = ref or R.reference(form, docs)
    assert np.array_equal(oo, ro), tag
    assert np.array_equal(ch, rc), tag
    got = out.cpu().numpy()
    assert got.shape == rd.shape, tag  # exactly `total` bytes
    if not np.array_equal(got, rd):
        w = np.nonzero(got != rd)[0]
        raise AssertionError("%s: %d bytes differ, the first at %d (chunk %d + %d): %d != %d" %
                             (tag, len(w), w[0], w[0] // _chunk(), w[0] % _chunk(), got[w[0]], rd[w[0]]))
    check(str(tag))


@pytest.mark.parametrize("out_shift", [0, 1, 5, 15])
def test_normalize_writes_an_output_off_the_boundary(normalizer, out_shift):
    C = _chunk()
    for name, docs in (("edges", R.edge_docs(C)), ("clean_behind_dirty", V.clean_behind_dirty("NFC", 5, 1, 17, C, many=True)[0])):
        for form in R.FORMS:
            _norm_check(normalizer, form, docs, 0, out_shift, (name, form, out_shift), _reference(name, form, docs))


@pytest.mark.parametrize("form", R.FORMS)
def test_clean_chunks_behind_a_dirty_one(normalizer, form):
    """k_norm_write's clean path through all sixteen residues of dst - src, every reachable front spill, and a short last
    chunk (head > n where the residues agree: delta = 16 with text and output shifted alike), as one document and with
    document boundaries inside the clean chunks (the clean path's out_offs loop).

    With head taken from src where it should be dst's, the first wrong byte is byte 0 of chunk 1's output for every
    delta but 16; with the head > n clamp gone, the guard behind the output of (delta 16, shift 1, last 1) is written."""
    C = _chunk()
    for m, sp, last in V.clean_behind_dirty_cases(form):
        for many in (False, True):
            docs, _want = V.clean_behind_dirty(form, m, sp, last, C, many=many)
            _norm_check(normalizer, form, docs, 0, 0, (form, m, sp, last, many))
            if m == 16:  # src and dst congruent again, both off the boundary: the head is 16 - s bytes
                for s in (1, 9, 15):
                    _norm_check(normalizer, form, docs, s, s, (form, m, sp, last, many, "shift", s))


# ---- 2. token spans -----------------------------------------------------------------------------------------------------
class SpanEnv:
    def __init__(self, oracle_mod, name):
        import torch
        self.name = name
        self.ctx, self.orc, self.is_byte = _shipped(oracle_mod, name)
        self.data, self.offs, ref_ids, ref_oo = V.spans_batch(self.orc)
        n, nb = len(self.offs) - 1, len(self.data)
        # the ids are the GPU's own, from an aligned copy of the text
        db, do = on16(dev(self.data.copy())), dev(self.offs)
        cap = self.ctx.ids_capacity(nb, n)
        ids = torch.zeros(cap, dtype=torch.int32, device=DEV)
        oo = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
        err = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        self.ctx.encode_device(db.data_ptr(), do.data_ptr(), n, nb, ids.data_ptr(), cap, oo.data_ptr(), 0, err.data_ptr(), 0)
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        self.oo = oo.cpu().numpy()
        self.ids = ids.cpu().numpy()[:int(self.oo[-1])]
        assert np.array_equal(self.ids, ref_ids) and np.array_equal(self.oo, ref_oo)
        assert len(self.ids) % V.SP_PER != 0 and nb % 16 != 0
        self.tt = S.TokenText(self.orc)
        self.want = {u: S.batch(self.tt, self.data, self.offs, self.ids, self.oo, self.is_byte, u, np.int64)[0] for u in ("byte", "char")}


@pytest.fixture(scope="module")
def span_envs(oracle_mod):
    envs = {name: SpanEnv(oracle_mod, name) for name in ("VG", "VL")}
    yield envs
    for e in envs.values():
        e.ctx.close()


def spans_call(env, unit, width, b_shift, i_shift, o_shift, data=None):
    """hutk_token_spans_device with the text b_shift bytes, the ids i_shift elements and the spans o_shift elements (of
    their width) off the boundary -> (spans [n_ids, 2], status, err), guards checked"""
    import torch
    data = env.data if data is None else data
    n, nb, n_ids = len(env.offs) - 1, len(data), len(env.ids)
    d_bytes = view(dev(data.copy()), b_shift)
    d_ids = view(dev(env.ids), i_shift)
    out, check = V.guarded(2 * n_ids, o_shift, tdtype(width), G32)
    (off16 if o_shift else on16)(out)
    d_offs, d_oo = dev(env.offs), dev(env.oo)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    err = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()  # (the call runs on the context's own stream)
    env.ctx.token_spans_device(d_bytes.data_ptr(), d_offs.data_ptr(), n, nb, d_ids.data_ptr(), d_oo.data_ptr(), n_ids,
                               0 if unit == "byte" else 1, width, out.data_ptr(), st.data_ptr(), err.data_ptr(), 0)
    torch.cuda.synchronize()
    check("%s spans %s int%d %s" % (env.name, unit, 8 * width, (b_shift, i_shift, o_shift)))
    return out.cpu().numpy().reshape(n_ids, 2), st.cpu().numpy(), int(err.item())


SPAN_SHIFTS = ([(b, 0, 0) for b in (1, 7, 8, 15)] + [(0, i, 0) for i in (1, 2, 3)] + [(0, 0, 1), (15, 3, 1)])


@pytest.mark.parametrize("name", ["VG", "VL"])
def test_spans_on_shifted_views(span_envs, name):
    """k_sp_bits' byte loop, sp_fetch's byte loads at both ends of the text (and its 8-byte loads from a base that is no
    multiple of 8), k_sp_tiles' element loads of the ids and element stores of the spans, both widths."""
    env = span_envs[name]
    for unit in ("byte", "char"):
        for width in (4, 8):
            twin, st, err = spans_call(env, unit, width, 0, 0, 0)
            assert err == 0 and not st.any() and np.array_equal(twin, env.want[unit]), (name, unit, width)
            for shifts in SPAN_SHIFTS:
                got, st, err = spans_call(env, unit, width, *shifts)
                tag = (name, unit, width, shifts)
                assert err == 0 and not st.any(), tag
                bad = np.nonzero((got != env.want[unit]).any(axis=1))[0]
                assert bad.size == 0, (tag, bad[:5], got[bad[:5]], env.want[unit][bad[:5]])
                assert np.array_equal(got, twin), tag


@pytest.mark.parametrize("name", ["VG", "VL"])
def test_tampered_text_at_the_end_of_a_shifted_buffer(span_envs, name):
    """The last byte of the text, inside the last token (at most 7 bytes, fetched byte by byte when the buffer ends off
    the boundary), is another letter: that document alone is a mismatch."""
    env = span_envs[name]
    n = len(env.offs) - 1
    victim = n - 2  # the last document is empty
    assert env.offs[victim + 1] == len(env.data) > env.offs[victim]
    bad = env.data.copy()
    bad[-1] = ord("x") if bad[-1] != ord("x") else ord("y")
    for unit in ("byte", "char"):
        for shift in (0, 1, 15):
            got, st, err = spans_call(env, unit, 4, shift, 0, 0, data=bad)
            assert err == E_UNSUPPORTED, (name, unit, shift)
            assert st[victim] == S.MISMATCH and int((st != 0).sum()) == 1, (name, unit, shift)
            keep = int(env.oo[victim])
            assert np.array_equal(got[:keep], env.want[unit][:keep]), (name, unit, shift)


# ---- 3. encoders --------------------------------------------------------------------------------------------------------
VL_MARKERS = {"<s>": 1, "</s>": 2, "<|eot_id|>": 32000}
ENCODERS = [("plain", 0), ("special", 0), ("fallback", 0), ("fallback", FB_SPECIAL)]


def _encode_fn(kind):
    from hutoken_amd import _capi
    L = _capi.load()
    return {"plain": L.hutk_encode_batch_device, "special": L.hutk_encode_special_batch_device,
            "fallback": L.hutk_encode_fallback_batch_device}[kind]


def encode_capi(ctx, kind, flags, d_bytes, d_offs, shift, fill=G32):
    """One of the three device encoders through the C ABI with d_ids_out `shift` elements off the boundary, in a guarded
    buffer of the least capacity the call accepts (its bound less one: it refuses anything below, the exact total too).
    -> (rc, the ids view as numpy, out_offsets, status, err)"""
    import torch
    n, nb = d_offs.numel() - 1, d_bytes.numel()
    cap = (ctx.special_ids_capacity if kind == "special" or flags else ctx.ids_capacity)(nb, n) - 1
    ids, check = V.guarded(cap, shift, torch.int32, fill)
    (off16 if shift else on16)(ids)
    oo = torch.full((n + 1,), -7, dtype=torch.int64, device=DEV)
    st = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    err = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = (ctx.handle, d_bytes.data_ptr(), d_offs.data_ptr(), n, nb) + ((flags,) if kind == "fallback" else ())
    torch.cuda.synchronize()  # (a NULL stream is the context's own: it waits for no torch stream)
    rc = _encode_fn(kind)(*args, ids.data_ptr(), cap, oo.data_ptr(), st.data_ptr(), err.data_ptr(), stream)
    torch.cuda.synchronize()
    check("%s encode, ids shifted by %d" % (kind, shift))
    return rc, ids.cpu().numpy(), oo.cpu().numpy(), st.cpu().numpy()[:n], int(err.item())


def _vl_texts():
    import random
    rng = random.Random(12)
    marks = list(VL_MARKERS)
    texts = ["<s>😂<|eot_id|>", "😂<s>漢", "", "<s>", "plain words only", "a</s>"]
    for _ in range(300):
        t = H.random_text(rng, max_words=12)
        cut = rng.randint(0, len(t))
        texts.append(rng.choice(marks + [""]) + t[:cut] + rng.choice(marks) + "😂" + t[cut:] + rng.choice(marks + [""]))
    return [t.encode("utf-8") for t in texts]


@pytest.fixture(scope="module")
def vl_encoders(oracle_mod, vl_files):
    """The package's own context on VL with special tokens and the byte-fallback table, and what its four encoders
    must give for one batch."""
    import hutoken_amd
    from oracle import oracle as O
    vp, sp, kw = vl_files
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    hutoken_amd.set_special_tokens(VL_MARKERS)
    hutoken_amd.set_byte_fallback("auto")
    ctx = hutoken_amd.context()
    orc = O.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    table = ctx.find_byte_tokens()[0]
    specials = {k.encode(): v for k, v in VL_MARKERS.items()}
    data, offs = R.pack(_vl_texts())
    tt = S.TokenText(orc)
    ids, oo, _st = orc.encode_packed(data, offs)
    assert (np.asarray(ids) == -1).any()
    want = {("plain", 0): (np.asarray(ids, dtype=np.int32), np.asarray(oo)),
            ("special", 0): SR.encode(orc, data, offs, specials)[:2],
            ("fallback", 0): F.encode(tt, data, offs, ids, oo, False, table)[:2],
            ("fallback", FB_SPECIAL): F.encode_special(orc, tt, data, offs, specials, False, table)[:2]}
    assert len({len(w[0]) for w in want.values()}) == 4
    yield ctx, data, offs, want
    hutoken_amd.set_special_tokens(None)
    hutoken_amd.set_byte_fallback(None)


def test_encoders_refuse_text_off_the_boundary(vl_encoders):
    """d_bytes & 15 != 0: HUTK_E_ARG from all three encoders, nothing written, nothing left behind in the context."""
    import hutoken_amd
    ctx, data, offs, want = vl_encoders
    aligned, do = on16(dev(data.copy())), dev(offs)
    bad = off16(V.shifted(aligned, 1))
    calls = {("plain", 0): lambda t: hutoken_amd.encode_packed_device(t, do),
             ("special", 0): lambda t: hutoken_amd.encode_special_packed_device(t, do),
             ("fallback", 0): lambda t: hutoken_amd.encode_fallback_packed_device(t, do),
             ("fallback", FB_SPECIAL): lambda t: hutoken_amd.encode_fallback_packed_device(t, do, special=True)}
    for (kind, flags) in ENCODERS:
        w_ids, w_oo = want[kind, flags]
        with pytest.raises(TypeError, match="16-byte aligned"):
            calls[kind, flags](bad)
        rc, ids, oo, st, err = encode_capi(ctx, kind, flags, bad, do, 0)
        assert rc == E_ARG, (kind, flags)
        assert (ids == G32).all() and (oo == -7).all() and (st == -7).all() and err == -7, (kind, flags)
        # the same context, the aligned copy: through the Python surface and through the C ABI
        g_ids, g_oo = calls[kind, flags](aligned)
        assert np.array_equal(g_oo.cpu().numpy(), w_oo), (kind, flags)
        assert np.array_equal(g_ids.cpu().numpy()[:len(w_ids)], w_ids), (kind, flags)
        rc, ids, oo, st, err = encode_capi(ctx, kind, flags, aligned, do, 0)
        assert rc == 0 and err == 0 and np.array_equal(oo, w_oo) and np.array_equal(ids[:len(w_ids)], w_ids), (kind, flags)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_encoders_write_ids_off_the_boundary(vl_encoders, shift):
    """d_ids_out aligned to its element only: the plain encoder, the fallback expansion and -- with markers in every
    document -- k_st_copy's four element stores per group."""
    ctx, data, offs, want = vl_encoders
    db, do = on16(dev(data.copy())), dev(offs)
    for (kind, flags) in ENCODERS:
        w_ids, w_oo = want[kind, flags]
        rc, ids, oo, st, err = encode_capi(ctx, kind, flags, db, do, shift)
        assert rc == 0 and err == 0 and not st.any(), (kind, flags, shift)
        assert np.array_equal(oo, w_oo), (kind, flags, shift)
        got = ids[:len(w_ids)]
        bad = np.nonzero(got != w_ids)[0]
        assert bad.size == 0, (kind, flags, shift, bad[:5], got[bad[:5]], w_ids[bad[:5]])
        rc, twin, _oo, _st, _err = encode_capi(ctx, kind, flags, db, do, 0)
        assert rc == 0 and np.array_equal(twin[:len(w_ids)], got), (kind, flags, shift)


@pytest.fixture(scope="module")
def special_case(oracle_mod):
    ctx, orc, _ = _shipped(oracle_mod, "VG")
    docs = V.special_batch(orc)
    data, offs = R.pack(docs)
    specials = {V.EOT: V.EOT_ID}
    ctx.set_special_tokens(sorted(specials.items()))
    w_ids, w_oo, w_st, matches = SR.encode(orc, data, offs, specials)
    assert not w_st.any() and matches >= len(docs)
    p_ids, p_oo, _ = orc.encode_packed(data, offs)
    yield ctx, data, offs, (w_ids, w_oo), (np.asarray(p_ids, dtype=np.int32), np.asarray(p_oo)), matches
    ctx.close()


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_special_copy_over_two_tiles_into_shifted_ids(special_case, shift):
    """k_st_copy with an output of two CP_TILE and a remainder that is no multiple of four: piece boundaries inside a
    group of four and exactly at the tile edge, every group written by element stores."""
    ctx, data, offs, (w_ids, w_oo), (p_ids, p_oo), matches = special_case
    assert 2 * V.CP_TILE < len(w_ids) and len(w_ids) % 4 != 0 and w_ids[V.CP_TILE - 1] == V.EOT_ID
    db, do = on16(dev(data.copy())), dev(offs)
    rc, ids, oo, st, err = encode_capi(ctx, "special", 0, db, do, shift)
    assert rc == 0 and err == 0 and not st.any() and ctx.special_last_matches == matches
    assert np.array_equal(oo, w_oo)
    got = ids[:len(w_ids)]
    bad = np.nonzero(got != w_ids)[0]
    assert bad.size == 0, (shift, bad[:5], got[bad[:5]], w_ids[bad[:5]])
    rc, ids, oo, st, err = encode_capi(ctx, "plain", 0, db, do, shift)  # the markers as text: the oracle's ids
    assert rc == 0 and err == 0 and np.array_equal(oo, p_oo) and np.array_equal(ids[:len(p_ids)], p_ids)


# ---- 4. decode of byte-fallback ids -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fb_decode(tmp_path_factory, oracle_mod):
    from test_gpu_fallback import _char_ctx
    ctx, _orc, ents, special = _char_ctx(tmp_path_factory.mktemp("views_fb"), oracle_mod, "őű漢")
    table = ctx.find_byte_tokens()[0]
    assert np.array_equal(table, V.byte_table(ents))
    ctx.set_byte_fallback(table)
    specials = [(b"<|eot|>", len(ents) + 5), (b"<s>", 300)]
    ctx.set_special_tokens(specials)
    tokens = F.from_decode_ref(DR.DecodeRef(ents, special, "▁", False))
    yield ctx, ents, table, specials, tokens
    ctx.close()


def fallback_device_call(ctx, ids, offs, total, flags, ids_shift=0, out_shift=0, tail=64):
    """device_call of tests/test_gpu_decode_special.py for Context.decode_fallback_device: the ids a view `ids_shift`
    elements into a larger tensor, the output `out_shift` bytes into a buffer of GUARD bytes with `tail` more behind.
    -> (the whole output buffer, out_offsets, status, err) as numpy"""
    import torch
    from test_gpu_decode_special import GUARD
    n, nd = len(ids), len(offs) - 1
    d_ids = view(dev(np.ascontiguousarray(ids, dtype=np.int32)), ids_shift)
    d_offs = dev(np.ascontiguousarray(offs, dtype=np.int64))
    buf = torch.full((out_shift + total + tail,), GUARD, dtype=torch.uint8, device=DEV)
    if out_shift:
        assert (buf.data_ptr() + out_shift) % 16 != 0
    d_oo = torch.full((nd + 1,), -1, dtype=torch.int64, device=DEV)
    d_st = torch.full((max(nd, 1),), -1, dtype=torch.int32, device=DEV)
    d_err = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()  # (the call runs on the context's own stream)
    ctx.decode_fallback_device(d_ids.data_ptr(), d_offs.data_ptr(), nd, n, flags, buf.data_ptr() + out_shift, total,
                               d_oo.data_ptr(), d_st.data_ptr(), d_err.data_ptr(), 0)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), d_oo.cpu().numpy(), d_st.cpu().numpy()[:nd], int(d_err.item())


@pytest.mark.parametrize("special", [False, True])
def test_fallback_decode_on_shifted_views(fb_decode, special):
    """k_fb_remap's element loads: FBR_TILE + 1 ids with table ids in the first two groups of four and on both sides of
    the pass's tile edge."""
    from test_gpu_decode_special import GUARD, first_diff
    ctx, ents, table, specials, tokens = fb_decode
    ids, offs = V.fallback_decode_batch(ents, table, [i for _k, i in specials] if special else ())
    assert len(ids) == V.FBR_TILE + 1 and all(ids[at] in table for at in V.FB_TABLE_AT)
    want, want_oo, want_st = F.decode_packed(tokens, ids, offs, table, specials if special else None, False)
    assert not want_st.any()
    total = len(want)
    flags = FB_SPECIAL if special else 0
    for ids_shift, out_shift in [(0, 0)] + [(i, o) for i in (1, 2, 3) for o in (1, 3, 15)]:
        buf, oo, st, err = fallback_device_call(ctx, ids, offs, total, flags, ids_shift, out_shift)
        what = "special=%s ids_shift=%d out_shift=%d" % (special, ids_shift, out_shift)
        assert err == 0 and not st.any(), what
        assert np.array_equal(oo, want_oo), "%s: out_offsets, %s" % (what, first_diff(oo, want_oo))
        got = buf[out_shift:out_shift + total]
        assert np.array_equal(got, want), "%s: bytes, %s" % (what, first_diff(got, want))
        assert (buf[:out_shift] == GUARD).all() and (buf[out_shift + total:] == GUARD).all(), what + ": bytes outside the output"


# ---- 5. padded and packed collation -------------------------------------------------------------------------------------
TOKENS = [{}, {"bos_id": -5, "eos_id": 50256}]
PAD = -9


def _tok(kw, key):
    from hutoken_amd import _capi
    return kw.get(key, _capi.NO_TOKEN)


def padded_call(ids, offs, kw, flags, width, which=(), ids_shift=0):
    """hutk_collate_padded_device with the outputs named in `which` one element off the boundary, each in a guarded buffer
    -> (input_ids [n, L], mask [n, L], lengths [n]) as numpy"""
    import torch
    from hutoken_amd import _capi
    n, L = len(offs) - 1, V.COLLATE_L
    d_ids, d_offs = view(dev(ids), ids_shift), dev(offs)
    bufs, checks = {}, []
    for name, count, dtype, guard in (("input_ids", n * L, tdtype(width), G32), ("mask", n * L, torch.uint8, V.GUARD_BYTE),
                                      ("lengths", n, torch.int32, G32)):
        shift = 1 if name in which else 0
        bufs[name], check = V.guarded(count, shift, dtype, guard)
        checks.append((name, check))
        if shift and name != "lengths":  # (lengths has no wide path: one element off is still its own alignment)
            assert bufs[name].data_ptr() % (16 if name == "input_ids" else 4) != 0
        elif not shift:
            on16(bufs[name])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _capi.collate_padded_device(d_ids.data_ptr(), d_offs.data_ptr(), n, len(ids), L, _tok(kw, "bos_id"), _tok(kw, "eos_id"),
                                PAD, flags, width, bufs["input_ids"].data_ptr(), bufs["mask"].data_ptr(),
                                bufs["lengths"].data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for name, check in checks:
        check("padded %s, shifted %s" % (name, which))
    return (bufs["input_ids"].cpu().numpy().reshape(n, L), bufs["mask"].cpu().numpy().reshape(n, L), bufs["lengths"].cpu().numpy())


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("width", [4, 8])
def test_padded_collation_on_shifted_views(width):
    """vec = L % 4 == 0 && input_ids 16-aligned && mask 4-aligned, with L = 64: each term false in turn, then all."""
    from hutoken_amd import _capi
    ids, offs = V.collate_batch()
    dtype = np.int32 if width == 4 else np.int64
    for kw in TOKENS:
        for flags in (0, _capi.COLLATE_TRUNC_LEFT, _capi.COLLATE_PAD_LEFT, _capi.COLLATE_TRUNC_LEFT | _capi.COLLATE_PAD_LEFT):
            want = CR.padded_vec(ids, offs, V.COLLATE_L, pad_id=PAD, dtype=dtype,
                                 truncation="left" if flags & _capi.COLLATE_TRUNC_LEFT else "right",
                                 padding_side="left" if flags & _capi.COLLATE_PAD_LEFT else "right", **kw)
            twin = padded_call(ids, offs, kw, flags, width)
            assert all(same(g, w) for g, w in zip(twin, want)), (kw, flags)
            for which in (("input_ids",), ("mask",), ("lengths",), ("input_ids", "mask", "lengths")):
                got = padded_call(ids, offs, kw, flags, width, which)
                assert all(same(g, w) for g, w in zip(got, want)), (kw, flags, which)
            for k in (1, 2, 3):
                got = padded_call(ids, offs, kw, flags, width, (), ids_shift=k)
                assert all(same(g, w) for g, w in zip(got, want)), (kw, flags, "ids", k)


ROW_KEYS = ("input_ids", "position_ids", "segment_ids")


def packed_call(ids, offs, kw, width, which=(), ids_shift=0):
    """Two hutk_packer_add_device calls (150 documents each: a row straddles them) and hutk_packer_flush_device, every
    output in a guarded buffer, those named in `which` one element off the boundary.
    -> (whole rows, flushed rows) as dicts of numpy arrays"""
    import torch
    from hutoken_amd import _capi
    L = V.COLLATE_L
    p = _capi.Packer(L, _tok(kw, "bos_id"), _tok(kw, "eos_id"), PAD, width, 0)
    dtype = np.int32 if width == 4 else np.int64
    st = torch.cuda.current_stream().cuda_stream

    def buffers(rows):
        out = {}
        for name in ROW_KEYS:
            shift = 1 if name in which else 0
            out[name] = V.guarded(rows * L, shift, tdtype(width) if name == "input_ids" else torch.int32, G32)
            (off16 if shift else on16)(out[name][0])
        return out

    def rows_of(bufs, n):
        for name in ROW_KEYS:
            bufs[name][1]("packed %s, shifted %s" % (name, which))
        return {name: bufs[name][0].cpu().numpy()[:n * L].reshape(n, L) for name in ROW_KEYS}

    parts = []
    n_docs = len(offs) - 1
    for a, b in ((0, n_docs // 2), (n_docs // 2, n_docs)):
        i, o = ids[int(offs[a]):int(offs[b])], offs[a:b + 1] - offs[a]
        d_i, d_o = view(dev(i), ids_shift), dev(o)
        rows = p.rows(len(o) - 1, len(i))
        bufs = buffers(rows)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        n = p.add(d_i.data_ptr(), d_o.data_ptr(), len(o) - 1, len(i), bufs["input_ids"][0].data_ptr(),
                  bufs["position_ids"][0].data_ptr(), bufs["segment_ids"][0].data_ptr(), rows, err.data_ptr(), st)
        torch.cuda.synchronize()
        assert int(err.item()) == 0 and n == rows
        parts.append(rows_of(bufs, n))
    assert p.pending > 0
    bufs = buffers(1)
    n = p.flush(bufs["input_ids"][0].data_ptr(), bufs["position_ids"][0].data_ptr(), bufs["segment_ids"][0].data_ptr(), st)
    torch.cuda.synchronize()
    assert n == 1 and p.pending == 0
    tail = rows_of(bufs, 1)
    p.close()
    return CR.cat_rows(parts, L, dtype), tail


@pytest.mark.parametrize("width", [4, 8])
def test_packed_collation_on_shifted_views(width):
    """vec = L % 4 == 0 && input_ids, position_ids and segment_ids 16-aligned, in k_collate_packed and in the flush."""
    ids, offs = V.collate_batch()
    dtype = np.int32 if width == 4 else np.int64
    for kw in TOKENS:
        want, want_tail = CR.packed_vec(ids, offs, V.COLLATE_L, pad_id=PAD, dtype=dtype, **kw)
        assert len(want_tail["input_ids"]) == 1
        twin, twin_tail = packed_call(ids, offs, kw, width)
        assert CR.rows_equal(twin, want) and CR.rows_equal(twin_tail, want_tail), kw
        for which in (("input_ids",), ("position_ids",), ("segment_ids",), ROW_KEYS):
            got, tail = packed_call(ids, offs, kw, width, which)
            assert CR.rows_equal(got, want) and CR.rows_equal(tail, want_tail), (kw, which)
        for k in (1, 2, 3):
            got, tail = packed_call(ids, offs, kw, width, (), ids_shift=k)
            assert CR.rows_equal(got, want) and CR.rows_equal(tail, want_tail), (kw, "ids", k)
