"""The decode kernels (hutk_decode.hip) where their paths change: tiles whose text is around 65536 bytes (16- and 32-bit
positions), around the 24576 bytes that are staged in LDS, every inline length at every alignment, tile counts around the
look-back window, empty documents on tile boundaries, stripped first tokens on every bit of the first-token words, the
device entry point with unaligned ids and output, and the per-document status of every kind of error.

Every case is compared bit for bit (bytes, out_offsets, status) with tests/decode_ref.py, through Context.decode_packed
and through Context.decode_device with torch tensors, and a seeded sample of its documents with the CPU oracle.
tests/test_decode_cpu.py checks the reference and the cases' sizes without a GPU.  Needs a real MI355X."""
import random
from collections import Counter

import numpy as np
import pytest

import decode_cases as DC
import helpers as H
from decode_ref import DecodeRef

pytestmark = pytest.mark.gpu

GUARD = 0xA5
E_VALUE, E_UNSUPPORTED, E_CAPACITY = 2, 6, 7


class Env:
    def __init__(self, v, tmp, name, oracle_mod):
        from hutoken_amd import _capi
        vp, sp = v.write(tmp, name)
        self.v, self.ref = v, v.ref
        self.ctx = _capi.Context(vp, sp, v.prefix, v.is_byte)
        self.orc = oracle_mod.Oracle(vp, sp, v.prefix, v.is_byte)


@pytest.fixture(scope="module")
def envs(tmp_path_factory, oracle_mod):
    tmp = tmp_path_factory.mktemp("decode_edges")
    return {"byte": Env(DC.Vocab("byte"), tmp, "b", oracle_mod), "char": Env(DC.Vocab("char"), tmp, "c", oracle_mod),
            "bytepfx": Env(DC.Vocab("byte", prefix="Ġ"), tmp, "p", oracle_mod)}


def device_call(ctx, ids, offs, total, ids_shift=0, out_shift=0, write=True, cap=None, tail=64):
    """Context.decode_device on torch tensors: the ids a view `ids_shift` elements into a larger tensor, the output
    `out_shift` bytes into a buffer of GUARD bytes with `tail` more of them behind.
    -> (the whole output buffer, out_offsets, status, err) as numpy"""
    import torch
    dev = "cuda:0"
    n, nd = len(ids), len(offs) - 1
    ids_buf = torch.zeros(n + 8, dtype=torch.int32, device=dev)
    d_ids = ids_buf[ids_shift:ids_shift + n]
    d_ids.copy_(torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)))
    d_offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int64)).to(dev)
    buf = torch.full((out_shift + total + tail,), GUARD, dtype=torch.uint8, device=dev)
    d_oo = torch.full((nd + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((max(nd, 1),), -1, dtype=torch.int32, device=dev)
    d_err = torch.full((1,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (the call runs on the context's own stream)
    ctx.decode_device(d_ids.data_ptr() if n else 0, d_offs.data_ptr(), nd, n, buf.data_ptr() + out_shift if write else 0,
                      total if cap is None else cap, d_oo.data_ptr(), d_st.data_ptr(), d_err.data_ptr(), 0)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), d_oo.cpu().numpy(), d_st.cpu().numpy()[:nd], int(d_err.item())


def first_diff(a, b):
    if len(a) != len(b):
        return "lengths %d != %d" % (len(a), len(b))
    w = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return "equal" if not len(w) else "first difference at index %d: %d != %d (%d differ)" % (w[0], a[w[0]], b[w[0]], len(w))


def check(env, name, ids, offs, rng=None, host=True, **dev_kw):
    """One batch through both entry points against the reference; a sample of documents against the oracle."""
    want, want_oo = env.ref.decode_packed(ids, offs)
    want_st = env.ref.status(ids, offs)
    total = len(want)
    assert not want_st.any(), name
    if host:
        out, oo, st = env.ctx.decode_packed(ids, offs)
        assert np.array_equal(oo, want_oo), "%s: host out_offsets, %s" % (name, first_diff(oo, want_oo))
        assert np.array_equal(out, want), "%s: host bytes, %s" % (name, first_diff(out, want))
        assert not st.any(), name
    shift = dev_kw.get("out_shift", 0)
    buf, oo, st, err = device_call(env.ctx, ids, offs, total, **dev_kw)
    assert err == 0, name
    assert np.array_equal(oo, want_oo), "%s: device out_offsets, %s" % (name, first_diff(oo, want_oo))
    assert not st.any(), name
    got = buf[shift:shift + total]
    assert np.array_equal(got, want), "%s: device bytes, %s" % (name, first_diff(got, want))
    assert (buf[:shift] == GUARD).all() and (buf[shift + total:] == GUARD).all(), name + ": bytes outside the output"
    if rng is not None and len(offs) > 1:
        raw = got.tobytes()
        nd = len(offs) - 1
        for d in [0, nd - 1] + [rng.randrange(nd) for _ in range(6)]:
            if offs[d + 1] - offs[d] <= 2 * DC.TILE + 2:  # (the oracle takes seconds for a document of 100 k ids)
                ref_bytes, st1 = env.orc.decode_bytes(ids[offs[d]:offs[d + 1]])
                assert st1 == 0 and raw[oo[d]:oo[d + 1]] == ref_bytes, (name, d)


def test_tile_text_around_65536_bytes(envs):
    """A tile's positions are 16 bits wide up to 65535 bytes of text and 32 bits wide above: out_offsets of the
    documents in the tile and of the tile behind it (2048 run tokens of 31, 32 and 33 bytes; of 300 bytes).  With 16-bit
    positions alone the first wrong out_offsets are those of document 2047 of the 65567-byte tile of one-token documents
    (65536 bytes in front of it) and of document 219 of the 300-byte one."""
    rng = random.Random(1)
    for name, ids, offs in DC.tile_total_cases(envs["byte"].v):
        check(envs["byte"], name, ids, offs, rng)
    env = envs["bytepfx"]  # every document's first token one byte shorter: the same tiles a little below
    for name, ids, offs in DC.tile_total_cases(env.v):
        check(env, "prefix_" + name, ids, offs, rng)


def test_staging_threshold(envs):
    """Tiles of 24575 and 24576 bytes are staged in LDS, one of 24577 goes straight to memory; an unstaged tile of
    inline and blob tokens between two staged ones that end at odd addresses."""
    rng = random.Random(2)
    for name, ids, offs in DC.staging_cases(envs["char"].v):
        check(envs["char"], name, ids, offs, rng)


@pytest.fixture(scope="module")
def vg(vg_files, oracle_mod):
    from hutoken_amd import _capi
    vp, sp, kw = vg_files
    ref = DC.shipped_vocab_ref(vg_files)
    return (_capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"]), ref,
            oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]))


def test_unstaged_tiles_of_the_shipped_vocabulary(vg):
    """VG has 2000 tokens of 13 bytes and more: tiles drawn from them are not staged (three of them here, between
    staged tiles)."""
    ctx, ref, orc = vg
    ids, offs = DC.shipped_vocab_case(ref)
    tot = np.add.reduceat(ref.lengths(ids, offs), np.arange(0, len(ids), DC.TILE))
    assert (tot > DC.STAGE).sum() >= 2 and (tot <= DC.STAGE).sum() >= 2
    env = type("E", (), {"ctx": ctx, "ref": ref, "orc": orc})
    check(env, "vg_long_tokens", ids, offs, random.Random(4))


def test_inline_lengths(envs):
    """Decoded lengths 0 .. 8 (inline up to 7 bytes, written as 4 + 2 + 1; 8 from the blob) at every alignment."""
    rng = random.Random(3)
    for kind in ("char", "byte"):
        for name, ids, offs in DC.inline_cases(envs[kind].v):
            check(envs[kind], kind + "_" + name, ids, offs, rng)


@pytest.mark.parametrize("help_after", ["default", "0"])
@pytest.mark.parametrize("n", DC.SIZES)
def test_tile_counts_and_document_boundaries(envs, monkeypatch, n, help_after):
    """n ids as one document, cut around every tile boundary, with runs of empty documents at the front, on a tile
    boundary and at the end; with the look-back waiting for its predecessors and adding their bytes up itself."""
    if help_after != "default":
        monkeypatch.setenv("HUTK_DEC_HELP_AFTER", help_after)
    rng = random.Random(n)
    for name, ids, offs in DC.size_cases(envs["byte"].v, n):
        check(envs["byte"], name, ids, offs, rng)
    if n in (2048, 2049, 64 * 2048 + 1):  # the first-token bitmap and stripped lengths at the same sizes
        for name, ids, offs in DC.size_cases(envs["char"].v, n):
            check(envs["char"], "char_" + name, ids, offs, rng)


@pytest.mark.parametrize("help_after", ["default", "0"])
def test_many_documents_in_one_tile(envs, monkeypatch, help_after):
    if help_after != "default":
        monkeypatch.setenv("HUTK_DEC_HELP_AFTER", help_after)
    for kind in ("byte", "char"):
        for name, ids, offs in DC.one_id_docs(envs[kind].v):
            check(envs[kind], kind + "_" + name, ids, offs, random.Random(5))


def test_prefix_stripping(envs):
    """First tokens on every bit of the first-token words and on a tile's first and last slot: the prefix alone (nothing
    left), three prefixes, a 100-character token with the prefix (stripped form in the blob) and one without."""
    rng = random.Random(6)
    for kind in ("char", "bytepfx"):
        for name, ids, offs in DC.prefix_cases(envs[kind].v):
            check(envs[kind], kind + "_" + name, ids, offs, rng)


def _mixed_batch(env):
    """a staged tile, an unstaged one, a staged one (tests/decode_cases.py: they meet at odd addresses)"""
    return DC.staging_cases(env.v)[-1][1:]


@pytest.mark.parametrize("ids_shift", [0, 1, 2, 3])
def test_device_ids_not_16_byte_aligned(envs, ids_shift):
    """d_ids a view 1, 2 and 3 elements into a tensor: the scalar loads instead of the 16-byte ones."""
    env = envs["char"]
    ids, offs = _mixed_batch(env)
    check(env, "ids_shift%d" % ids_shift, ids, offs, host=False, ids_shift=ids_shift)
    ids, offs = DC.size_cases(envs["byte"].v, 2049)[1][1:]
    check(envs["byte"], "ids_shift%d_2049" % ids_shift, ids, offs, host=False, ids_shift=ids_shift)


@pytest.mark.parametrize("out_shift", [1, 3, 8, 15])
def test_device_output_misaligned(envs, out_shift):
    """d_bytes_out needs no alignment: the partial first and last 16-byte chunks of the staged tiles and the unstaged
    tile's byte stores leave the bytes in front of the output and behind its end alone."""
    env = envs["char"]
    ids, offs = _mixed_batch(env)
    check(env, "out_shift%d" % out_shift, ids, offs, host=False, out_shift=out_shift)
    for name, ids, offs in DC.tile_total_cases(envs["byte"].v)[2:4]:  # (the tile of 65536 bytes)
        check(envs["byte"], "out_shift%d_%s" % (out_shift, name), ids, offs, host=False, out_shift=out_shift,
              ids_shift=out_shift % 4)


def test_device_sizes_only_and_capacity(envs):
    """d_bytes_out = 0: the same out_offsets and status.  bytes_cap one short: HUTK_E_CAPACITY in d_err, nothing
    written at or beyond bytes_cap, the tiles that fit are written; the host call raises."""
    from hutoken_amd import _capi
    env = envs["char"]
    ids, offs = _mixed_batch(env)
    want, want_oo = env.ref.decode_packed(ids, offs)
    total = len(want)
    buf, oo, st, err = device_call(env.ctx, ids, offs, total, write=False)
    assert err == 0 and np.array_equal(oo, want_oo) and not st.any()
    assert (buf == GUARD).all()
    buf, oo, st, err = device_call(env.ctx, ids, offs, total, cap=total - 1, out_shift=3)
    assert err == E_CAPACITY
    assert np.array_equal(oo, want_oo) and not st.any()
    assert (buf[:3] == GUARD).all() and (buf[3 + total - 1:] == GUARD).all()
    tile_end = np.cumsum(np.add.reduceat(env.ref.lengths(ids, offs), np.arange(0, len(ids), DC.TILE)))
    fits = int(tile_end[tile_end <= total - 1].max())  # the last tile does not fit and writes nothing
    assert 0 < fits < total and np.array_equal(buf[3:3 + fits], want[:fits]) and (buf[3 + fits:] == GUARD).all()
    L = _capi.load()
    out = np.full(total + 8, GUARD, dtype=np.uint8)
    oo = np.zeros(len(offs), dtype=np.int64)
    st = np.zeros(len(offs), dtype=np.int32)
    ids32 = np.ascontiguousarray(ids, dtype=np.int32)
    rc = L.hutk_decode_batch(env.ctx._h, ids32.ctypes.data, offs.ctypes.data, len(offs) - 1, out.ctypes.data, total - 1,
                             oo.ctypes.data, st.ctypes.data)
    assert rc == E_CAPACITY
    with pytest.raises(RuntimeError, match="bytes_cap too small"):
        _capi.raise_for(rc)
    assert (out == GUARD).all()
    check(env, "after_capacity_error", ids, offs)  # the context decodes exactly again


@pytest.fixture(scope="module")
def err_env(tmp_path_factory, oracle_mod):
    """a vocabulary with ids that two keys carry and ids that none carries"""
    from hutoken_amd import _capi
    ents, special = H.random_byte_vocab(8, n_merges=100, dup_ids=True)
    vp, sp = H.write_vocab(tmp_path_factory.mktemp("decode_err"), "e", ents, special)
    cnt = Counter(i for _k, i in ents)
    env = type("E", (), {})()
    env.ctx, env.ref = _capi.Context(vp, sp, None, True), DecodeRef(ents, special, None, True)
    env.orc = oracle_mod.Oracle(vp, sp, None, True)
    env.good = np.asarray([i for i in range(len(ents)) if cnt[i] == 1], dtype=np.int32)
    env.bad = {"out_of_range": [len(ents), -1, 2 ** 31 - 1], "two_keys": [i for i, c in cnt.items() if c > 1][:3],
               "no_key": [i for i in range(len(ents)) if i not in cnt][:3]}
    return env


@pytest.mark.parametrize("kind,code,doc_code,message", [
    ("out_of_range", E_VALUE, 3, "non-negative and less than vocab size"),
    ("two_keys", E_UNSUPPORTED, 4, "cannot be decoded on its own"),
    ("no_key", E_UNSUPPORTED, 4, "cannot be decoded on its own")], ids=["out_of_range", "two_keys", "no_key"])
def test_error_statuses(err_env, kind, code, doc_code, message):
    """One kind of bad id per call, in the first, a middle and the last document, in a document that spans three tiles
    and in one between empty documents: status[] names exactly those documents, d_err the call's code, the other
    documents decode as ever, and the next clean call is exact."""
    env = err_env
    rng = np.random.default_rng(11)
    lens = [50, 0, 30, 700, 0, 9, 0, 1500, 2 * DC.TILE + 100, 40, 0, 0, 300, 25]  # document 8 spans tiles 1 .. 3
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    clean = rng.choice(env.good, int(offs[-1])).astype(np.int32)
    places = {"first": [0], "middle": [7], "last": [13], "three_tiles": [8], "between_empty": [5], "several": [0, 5, 8, 13]}
    for place, docs in places.items():
        ids = clean.copy()
        for j, d in enumerate(docs):
            at = int(offs[d]) + (int(rng.integers(0, lens[d])) if d != 8 else DC.TILE + 1000)  # (8: in its middle tile)
            ids[at] = env.bad[kind][j % len(env.bad[kind])]
        want, want_oo = env.ref.decode_packed(ids, offs)
        want_st = env.ref.status(ids, offs)
        assert np.nonzero(want_st)[0].tolist() == docs and (want_st[docs] == doc_code).all()
        buf, oo, st, err = device_call(env.ctx, ids, offs, len(want))
        assert err == code, (kind, place)
        assert np.array_equal(st, want_st), (kind, place, st.tolist())
        assert np.array_equal(oo, want_oo), "%s %s: %s" % (kind, place, first_diff(oo, want_oo))
        assert np.array_equal(buf[:len(want)], want) and (buf[len(want):] == GUARD).all(), (kind, place)
        with pytest.raises(ValueError, match=message):
            env.ctx.decode_packed(ids, offs)
        check(env, "clean_after_%s_%s" % (kind, place), clean, offs, random.Random(7))
