"""hutk_decode_special_batch_device / hutk_decode_special_batch (csrc/hutk_special.hip: k_dsp_remap in front of the decode
kernels) against tests/decode_special_ref.py, bit for bit -- bytes, out_offsets, status, error word -- through the device
call and the host call, with flags 0 and HUTK_DECODE_SKIP_SPECIAL unless a test says otherwise.  No document is ever left
out.  tests/test_decode_special_cpu.py pins the reference without a GPU.  Needs a real MI355X."""
import random

import numpy as np
import pytest

import decode_cases as DC
import decode_special_ref as DS
import helpers as H
from decode_ref import DecodeRef

pytestmark = pytest.mark.gpu

GUARD = 0xA5
E_VALUE, E_ARG, E_UNSUPPORTED, E_CAPACITY = 2, 4, 6, 7
OUT_OF_RANGE, UNDECODABLE = 3, 4
SKIP = 1  # HUTK_DECODE_SKIP_SPECIAL
TILE = DC.TILE
CODE_OF = {0: 0, OUT_OF_RANGE: E_VALUE, UNDECODABLE: E_UNSUPPORTED}


class Env:
    def __init__(self, v, tmp, name):
        from hutoken_amd import _capi
        vp, sp = v.write(tmp, name)
        self.v, self.ref = v, v.ref
        self.ctx = _capi.Context(vp, sp, v.prefix, v.is_byte)
        self.good = np.nonzero(~v.ref.bad)[0].astype(np.int32)
        # tokens whose form at the front of a document differs from the one inside
        self.prefixed = np.nonzero(~v.ref.bad & (v.ref.slen != v.ref.len))[0].astype(np.int32)

    def install(self, specials):
        self.ctx.set_special_tokens(specials)
        return specials


def _char_without_prefix():
    v = DC.Vocab("char")
    v.prefix = None
    v.ref = DecodeRef(v.entries, v.special, None, False)
    return v


@pytest.fixture(scope="module")
def envs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("decode_special")
    return {"byte": Env(DC.Vocab("byte"), tmp, "b"), "bytepfx": Env(DC.Vocab("byte", prefix="Ġ"), tmp, "p"),
            "char": Env(DC.Vocab("char"), tmp, "c"), "charnopfx": Env(_char_without_prefix(), tmp, "n")}


def device_call(ctx, ids, offs, total, flags, ids_shift=0, out_shift=0, write=True, cap=None, tail=64, plain=False):
    """Context.decode_special_device (plain: Context.decode_device) on torch tensors: the ids a view `ids_shift` elements
    into a larger tensor, the output `out_shift` bytes into a buffer of GUARD bytes with `tail` more of them behind.
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
    out = buf.data_ptr() + out_shift if write else 0
    if plain:
        ctx.decode_device(d_ids.data_ptr() if n else 0, d_offs.data_ptr(), nd, n, out, total if cap is None else cap,
                          d_oo.data_ptr(), d_st.data_ptr(), d_err.data_ptr(), 0)
    else:
        ctx.decode_special_device(d_ids.data_ptr() if n else 0, d_offs.data_ptr(), nd, n, flags, out,
                                  total if cap is None else cap, d_oo.data_ptr(), d_st.data_ptr(), d_err.data_ptr(), 0)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), d_oo.cpu().numpy(), d_st.cpu().numpy()[:nd], int(d_err.item())


def host_call(ctx, ids, offs, flags, total, cap=None):
    """hutk_decode_special_batch: the sizes call, then the text call (with room for `total` bytes, or `cap`)
    -> (rc, bytes and 8 guard bytes, out_offsets, status)"""
    from hutoken_amd import _capi
    L = _capi.load()
    ids32 = np.ascontiguousarray(ids, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    n = len(offs) - 1
    pid = ids32.ctypes.data if len(ids32) else None
    oo0 = np.full(n + 1, -1, dtype=np.int64)
    st = np.full(max(n, 1), -1, dtype=np.int32)
    rc0 = L.hutk_decode_special_batch(ctx.handle, pid, offs.ctypes.data, n, flags, None, 0, oo0.ctypes.data, st.ctypes.data)
    out = np.full(total + 8, GUARD, dtype=np.uint8)
    oo = np.full(n + 1, -1, dtype=np.int64)
    rc = L.hutk_decode_special_batch(ctx.handle, pid, offs.ctypes.data, n, flags, out.ctypes.data,
                                     total if cap is None else cap, oo.ctypes.data, st.ctypes.data)
    assert (rc0 == rc or cap is not None) and np.array_equal(oo0, oo)
    return rc, out, oo, st[:n]


def first_diff(a, b):
    if len(a) != len(b):
        return "lengths %d != %d" % (len(a), len(b))
    w = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return "equal" if not len(w) else "first difference at index %d: %d != %d (%d differ)" % (w[0], a[w[0]], b[w[0]], len(w))


def check(env, name, ids, offs, specials, skips=(False, True), host=True, **dev_kw):
    """One batch through both entry points and both flags against the reference.  A batch with bad ids: the error word
    and the documents' status are the reference's, every other token and document is exact."""
    ids = np.asarray(ids, dtype=np.int64)
    offs = np.asarray(offs, dtype=np.int64)
    want_st = DS.status(env.ref, ids, offs, specials)
    code = CODE_OF[int(want_st.max())] if len(want_st) else 0
    for skip in skips:
        what = "%s (skip=%s)" % (name, skip)
        want, want_oo = DS.decode_packed(env.ref, ids, offs, specials, skip)
        total = len(want)
        if host:
            rc, out, oo, st = host_call(env.ctx, ids, offs, SKIP if skip else 0, total)
            assert rc == code, what
            assert np.array_equal(oo, want_oo), "%s: host out_offsets, %s" % (what, first_diff(oo, want_oo))
            assert np.array_equal(st, want_st), what
            if code == 0:
                assert np.array_equal(out[:total], want), "%s: host bytes, %s" % (what, first_diff(out[:total], want))
            assert (out[total:] == GUARD).all(), what
        shift = dev_kw.get("out_shift", 0)
        buf, oo, st, err = device_call(env.ctx, ids, offs, total, SKIP if skip else 0, **dev_kw)
        assert err == code, what
        assert np.array_equal(oo, want_oo), "%s: device out_offsets, %s" % (what, first_diff(oo, want_oo))
        assert np.array_equal(st, want_st), what
        got = buf[shift:shift + total]
        assert np.array_equal(got, want), "%s: device bytes, %s" % (what, first_diff(got, want))
        assert (buf[:shift] == GUARD).all() and (buf[shift + total:] == GUARD).all(), what + ": bytes outside the output"


def general_set(n):
    """strings of 1, 7, 8 and 255 bytes; ids beyond the vocabulary, far beyond, 2**31 - 1, a vocabulary line (5) with
    other bytes, two strings with one id"""
    return [(b"<|endoftext|>", n), (b"\n", n + 1), (b"<|sep|>", n + 2), (b"<|im_st>", n + 9), (b"<|again|>", n),
            (b"y" * 255, 2**31 - 1), (b"<five>", 5), (b"<far>", 10**6)]


def special_ids(specials):
    return sorted(DS.strings(specials))


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["byte", "bytepfx", "char", "charnopfx"])
def test_random_batches(envs, kind):
    """About 2,000 documents of 0 .. 40 ids, about 15 % of them special, empty documents among them."""
    env = envs[kind]
    specials = env.install(general_set(env.ref.n))
    sids = special_ids(specials)
    rng = random.Random(31)
    good = [int(i) for i in env.good if int(i) not in sids]
    docs = [[rng.choice(sids) if rng.random() < 0.15 else rng.choice(good) for _ in range(rng.choice([0, 0] + list(range(41))))]
            for _ in range(2000)]
    ids, offs = DC.pack(docs)
    assert (np.diff(offs) == 0).sum() > 50 and 0.1 < np.isin(ids, sids).mean() < 0.2
    check(env, kind + "_random", ids, offs, specials)


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("help_after", ["default", "0"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 2047, 2048, 2049, 4097])
def test_word_and_tile_edges(envs, monkeypatch, n, help_after):
    """One document of n ids on a prefix vocabulary, a special at each of the positions 0, 31, 32, 2047, 2048 and n - 1
    that exist: the bit behind a special falls into the next 32-bit word and into the next tile.  Every ordinary token
    has a stripped form that differs from its plain one, so a bit that is missing, or one too many, changes the text."""
    if help_after != "default":
        monkeypatch.setenv("HUTK_DEC_HELP_AFTER", help_after)
    for kind in ("char", "bytepfx"):
        env = envs[kind]
        specials = env.install(general_set(env.ref.n))
        sids = special_ids(specials)
        rng = random.Random(n)
        pool = [int(i) for i in env.prefixed if int(i) not in sids]
        assert len(pool) >= 10
        ids = [rng.choice(pool) for _ in range(n)]
        if n == 1:  # (position 0 = n - 1 is a special below: the one token on its own first)
            check(env, "%s_n1_token" % kind, ids, [0, 1], specials)
        for j, p in enumerate(sorted({p for p in (0, 31, 32, 2047, 2048, n - 1) if p < n})):
            ids[p] = sids[j % len(sids)]
        check(env, "%s_n%d" % (kind, n), ids, [0, n], specials)


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def test_document_edges(envs):
    for kind in ("char", "bytepfx"):
        env = envs[kind]
        specials = env.install(general_set(env.ref.n))
        sids = special_ids(specials)
        rng = random.Random(33)
        pool = [int(i) for i in env.prefixed if int(i) not in sids]

        def tok(k):
            return [rng.choice(pool) for _ in range(k)]
        docs = [tok(3) + [sids[0]],      # a special as the last id of document d ...
                tok(4),                  # ... d + 1 starts on a prefix token: stripped once, whatever the special did
                tok(2) + [sids[1]], [], [], tok(2),          # empty documents in between
                [sids[0], sids[2], sids[1]],                 # only specials
                [sids[3]], tok(1), [], [sids[0]], [sids[0]], tok(5),
                [sids[0], sids[1]] + tok(3),                 # skip: the document's front moves over two specials
                [sids[2]], [], [sids[2], sids[2]], tok(1) + [sids[4]] + tok(1)]
        ids, offs = DC.pack(docs)
        fill = (-len(ids) - 1) % 32  # a special as the last id of the batch, n_ids a multiple of 32
        docs.append(tok(fill) + [sids[1]])
        ids, offs = DC.pack(docs)
        assert len(ids) % 32 == 0 and int(ids[-1]) == sids[1]
        check(env, kind + "_document_edges", ids, offs, specials)
        # the same at a tile's end: the last id of the batch is a special on slot 2047, and one on slot 4095
        for n in (TILE, 2 * TILE):
            docs = [tok(rng.randint(0, 9)) + [rng.choice(sids)] * rng.randint(0, 2) for _ in range(n // 4)]
            ids = [i for d in docs for i in d][:n - 1]
            ids += tok(n - 1 - len(ids)) + [sids[0]]
            cuts = sorted(rng.sample(range(1, n), 200)) + [n] * 3  # (empty documents at the end)
            check(env, "%s_last_of_batch_%d" % (kind, n), *DC.cut(ids, cuts), specials)


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def _exact_tile(env, rng, total, s255, s8):
    """2048 ids of one-byte and two-byte tokens, 8-byte and 255-byte specials whose text is exactly `total` bytes"""
    one = [int(i) for i in np.nonzero(~env.ref.bad & (env.ref.len == 1))[0][:50]]
    two = [int(i) for i in np.nonzero(~env.ref.bad & (env.ref.len == 2))[0][:50]]
    k = (total - TILE) // 254
    rest = total - TILE - 254 * k
    a, b = rest // 7, rest % 7
    assert k + a + b <= TILE
    ids = [s255] * k + [s8] * a + [rng.choice(two) for _ in range(b)]
    ids += [rng.choice(one) for _ in range(TILE - len(ids))]
    rng.shuffle(ids)
    return ids


def test_lengths(envs):
    """Special strings of 1, 7, 8 and 255 bytes (inline and blob entries); a tile of 2048 specials of 255 bytes (522,240
    bytes: not staged, 32-bit positions); tiles of a mixture just under and over the 24,576 bytes that are staged and the
    65,535 that 16-bit positions reach, one kind behind the other."""
    env = envs["byte"]
    n = env.ref.n
    specials = env.install([(b"\n", n), (b"<|sep|>", n + 1), (b"<|im_st>", n + 2), (b"y" * 127 + b"z" * 128, n + 3)])
    s1, s7, s8, s255 = n, n + 1, n + 2, n + 3
    rng = random.Random(34)
    ids = [s1, s7, s8, s255] * 5 + [int(rng.choice(env.good)) for _ in range(30)]
    rng.shuffle(ids)
    check(env, "each_length", *DC.cut_random(ids, rng, 0, 5), specials)
    check(env, "tile_of_255", [s255] * TILE + [s7, 1, 2], [0, 5, TILE, TILE + 3], specials)
    totals = [DC.STAGE - 1, DC.STAGE, DC.STAGE + 1, 65534, DC.STAGE, 65535, 65536, 65537, DC.STAGE - 7]
    ids = []
    for t in totals:
        ids += _exact_tile(env, rng, t, s255, s8)
    ids += [s255, s1, 3]
    per_id = np.diff(DS.decode_packed(env.ref, ids, np.arange(len(ids) + 1), specials)[1])  # (no prefix: no stripping)
    got = np.add.reduceat(per_id, np.arange(0, len(ids), TILE))
    assert got.tolist()[:len(totals)] == totals
    cuts = sorted(set(rng.sample(range(1, len(ids)), 300)) | {t * TILE for t in range(1, len(totals) + 1)})
    check(env, "tile_totals", *DC.cut(ids, cuts), specials)
    check(env, "tile_totals_one_doc", ids, [0, len(ids)], specials, host=False)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def err_env(tmp_path_factory):
    """a vocabulary with ids that two keys carry and ids that none carries"""
    from hutoken_amd import _capi
    ents, special = H.random_byte_vocab(8, n_merges=100, dup_ids=True)
    vp, sp = H.write_vocab(tmp_path_factory.mktemp("decode_special_err"), "e", ents, special)
    env = type("E", (), {})()
    env.ctx, env.ref = _capi.Context(vp, sp, None, True), DecodeRef(ents, special, None, True)
    env.good = np.nonzero(~env.ref.bad)[0].astype(np.int32)
    env.undecodable = [int(i) for i in np.nonzero(env.ref.bad)[0]]
    return env


def test_id_classes(err_env):
    env = err_env
    n = env.ref.n
    dup, other_dup = env.undecodable[0], env.undecodable[1]
    specials = [(b"<five>", 5), (b"<far>", 10**6), (b"<max>", 2**31 - 1), (b"<one>", n + 44), (b"<two>", n + 44),
                (b"<dup>", dup)]
    env.ctx.set_special_tokens(specials)
    sids = special_ids(specials)
    assert len(sids) == 5 and not set(range(n, n + 5)) & set(sids)
    rng = random.Random(35)
    good = [int(i) for i in env.good if int(i) not in sids]
    docs = [[rng.choice(sids) if rng.random() < 0.3 else rng.choice(good) for _ in range(rng.randint(0, 30))]
            for _ in range(300)]
    docs[7] = [5, dup, 2**31 - 1, n + 44, 10**6] * 3  # every class in one document
    ids, offs = DC.pack(docs)
    check(env, "every_class", ids, offs, specials)
    want = DS.decode_packed(env.ref, ids, offs, specials)[0].tobytes()
    assert b"<five><dup><max><one><far><five>" in want and b"<two>" not in want
    # ids that are neither special nor vocabulary lines: in [n_vocab, n_vocab + n_special), above it, negative
    for bad in (n, n + 1, n + 4, n + 5, n + 43, n + 45, 10**6 - 1, 2**31 - 2, -1, -2**31):
        for d in (0, 150, 299):
            mine = [list(x) for x in docs]
            mine[d] = mine[d][:3] + [bad] + mine[d][3:]
            ids, offs = DC.pack(mine)
            want_st = DS.status(env.ref, ids, offs, specials)
            assert np.nonzero(want_st)[0].tolist() == [d] and want_st[d] == OUT_OF_RANGE
            check(env, "bad_id_%d_doc%d" % (bad, d), ids, offs, specials, host=(d == 150))
    # an ordinary id that cannot be decoded on its own stays what it is in the plain decode
    mine = [list(x) for x in docs]
    mine[11] = [other_dup] + mine[11]
    ids, offs = DC.pack(mine)
    assert DS.status(env.ref, ids, offs, specials)[11] == UNDECODABLE
    check(env, "undecodable", ids, offs, specials)
    check(env, "clean_again", *DC.pack(docs), specials)


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_set_lifecycle(envs):
    from hutoken_amd import _capi
    env = envs["char"]
    n = env.ref.n
    rng = random.Random(36)
    env.ctx.set_special_tokens([])
    ids = [int(rng.choice(env.good)) for _ in range(3000)]
    ids[100], ids[2500] = n, -1  # (no set: ids beyond the vocabulary are out of range)
    ids, offs = DC.cut_random(ids, rng, 0, 30)
    total = len(env.ref.decode_packed(ids, offs)[0])
    plain = device_call(env.ctx, ids, offs, total, 0, plain=True)
    assert plain[3] == E_VALUE and (plain[2] == OUT_OF_RANGE).sum() == 2
    for flags in (0, SKIP):
        got = device_call(env.ctx, ids, offs, total, flags)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], plain[:3])) and got[3] == plain[3], flags
    check(env, "no_set", ids, offs, [])
    # a set; another one in its place; none
    first = env.install([(b"<a>", n), (b"<b>", n + 1)])
    ids = [int(rng.choice(env.prefixed)) if rng.random() < 0.8 else n + rng.randint(0, 1) for _ in range(3000)]
    ids, offs = DC.cut_random(ids, rng, 0, 30)
    check(env, "first_set", ids, offs, first)
    second = env.install([(b"<other>", n + 1), (b"<|a much longer string|>", n + 2)])
    ids[5] = n + 2
    ids = np.where(ids == n, n + 2, ids)
    check(env, "second_set", ids, offs, second)
    with pytest.raises(ValueError):  # a refused set leaves the tables in force
        env.ctx.set_special_tokens([(b"", 1)])
    check(env, "after_refused_set", ids, offs, second)
    # the plain decode never looks at the set
    ok = np.where(ids >= n, int(env.prefixed[0]), ids)
    out, oo, st = env.ctx.decode_packed(ok, offs)
    want, want_oo = env.ref.decode_packed(ok, offs)
    assert np.array_equal(out, want) and np.array_equal(oo, want_oo) and not st.any()
    with pytest.raises(ValueError, match="less than vocab size"):
        env.ctx.decode_packed(ids, offs)
    buf, oo, st, err = device_call(env.ctx, ids, offs, len(want), 0, plain=True)
    assert err == E_VALUE and np.array_equal(st, env.ref.status(ids, offs))
    env.ctx.set_special_tokens([])
    assert env.ctx.special_token_count == 0
    check(env, "set_removed", ids, offs, [])  # (n + 1, n + 2: out of range again)
    assert _capi.OK == 0


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def _mixed(env, specials, seed=37):
    """three tiles and a partial one: ordinary ids, a tile with many long specials (not staged), ordinary ids"""
    rng = random.Random(seed)
    sids = special_ids(specials)
    pool = [int(i) for i in env.prefixed if int(i) not in sids]
    ids = [rng.choice(sids) if rng.random() < 0.1 else rng.choice(pool) for _ in range(TILE)]
    ids += [2**31 - 1 if rng.random() < 0.3 else rng.choice(pool) for _ in range(TILE)]
    ids += [rng.choice(sids) if rng.random() < 0.1 else rng.choice(pool) for _ in range(TILE + 77)]
    ids, offs = DC.cut_random(ids, rng, 0, 90)
    return ids, np.unique(np.concatenate([offs, [TILE, 2 * TILE, 3 * TILE]]))  # documents end with the tiles


def test_sizes_capacity_and_alignment(envs):
    env = envs["char"]
    specials = env.install(general_set(env.ref.n))
    ids, offs = _mixed(env, specials)
    for skip in (False, True):
        flags = SKIP if skip else 0
        want, want_oo = DS.decode_packed(env.ref, ids, offs, specials, skip)
        total = len(want)
        buf, oo, st, err = device_call(env.ctx, ids, offs, total, flags, write=False)
        assert err == 0 and np.array_equal(oo, want_oo) and not st.any() and (buf == GUARD).all()
        buf, oo, st, err = device_call(env.ctx, ids, offs, total, flags, cap=total - 1, out_shift=3)
        assert err == E_CAPACITY and np.array_equal(oo, want_oo) and not st.any()
        assert (buf[:3] == GUARD).all() and (buf[3 + total - 1:] == GUARD).all()
        fits = int(want_oo[np.searchsorted(offs, 3 * TILE)])  # the last tile does not fit and writes nothing
        assert 0 < fits < total and np.array_equal(buf[3:3 + fits], want[:fits]) and (buf[3 + fits:] == GUARD).all()
        rc, out, oo, st = host_call(env.ctx, ids, offs, flags, total, cap=total - 1)
        assert rc == E_CAPACITY and np.array_equal(oo, want_oo) and (out == GUARD).all()
    check(env, "after_capacity_error", ids, offs, specials)
    for ids_shift in (1, 2, 3):
        check(env, "ids_shift%d" % ids_shift, ids, offs, specials, host=False, ids_shift=ids_shift)
    for out_shift in (1, 3, 15):
        check(env, "out_shift%d" % out_shift, ids, offs, specials, host=False, out_shift=out_shift, ids_shift=out_shift % 4)


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_arguments(envs):
    import torch
    from hutoken_amd import _capi
    L = _capi.load()
    env = envs["byte"]
    env.install(general_set(env.ref.n))
    h = env.ctx.handle
    dev = "cuda:0"
    d_ids = torch.zeros(8, dtype=torch.int32, device=dev)
    d_offs = torch.tensor([0, 8], dtype=torch.int64, device=dev)
    d_oo = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dev_call = L.hutk_decode_special_batch_device
    p, o, q = d_ids.data_ptr(), d_offs.data_ptr(), d_oo.data_ptr()
    assert dev_call(None, p, o, 1, 8, 0, None, 0, q, None, None, None) == E_ARG      # NULL context
    for flags in (2, 3, 4, -1, 1 << 30):
        assert dev_call(h, p, o, 1, 8, flags, None, 0, q, None, None, None) == E_ARG  # unknown flag bits
    assert dev_call(h, p, None, 1, 8, 0, None, 0, q, None, None, None) == E_ARG      # NULL id_offsets
    assert dev_call(h, p, o, 1, 8, 0, None, 0, None, None, None, None) == E_ARG      # NULL out_offsets
    assert dev_call(h, None, o, 1, 8, 0, None, 0, q, None, None, None) == E_ARG      # NULL ids, n_ids > 0
    assert dev_call(h, p, o, -1, 8, 0, None, 0, q, None, None, None) == E_ARG
    assert dev_call(h, p, o, 1, -8, 0, None, 0, q, None, None, None) == E_ARG
    assert dev_call(h, p, o, 1, 8, 2, None, 0, q, None, None, None) == E_ARG
    assert "unknown flags" in _capi.last_error()
    assert dev_call(h, None, o, 1, 0, 0, None, 0, q, None, None, None) == 0          # NULL ids with n_ids == 0; sizes only
    torch.cuda.synchronize()
    assert d_oo.tolist() == [0, 0]
    host = L.hutk_decode_special_batch
    ids, offs, oo = np.zeros(8, np.int32), np.array([0, 8], np.int64), np.zeros(2, np.int64)
    assert host(None, ids.ctypes.data, offs.ctypes.data, 1, 0, None, 0, oo.ctypes.data, None) == E_ARG
    assert host(h, ids.ctypes.data, offs.ctypes.data, 1, 2, None, 0, oo.ctypes.data, None) == E_ARG
    assert host(h, ids.ctypes.data, None, 1, 0, None, 0, oo.ctypes.data, None) == E_ARG
    assert host(h, ids.ctypes.data, offs.ctypes.data, 1, 0, None, 0, None, None) == E_ARG
    assert host(h, None, offs.ctypes.data, 1, 0, None, 0, oo.ctypes.data, None) == E_ARG
    bad = np.array([1, 8], np.int64)
    assert host(h, ids.ctypes.data, bad.ctypes.data, 1, 0, None, 0, oo.ctypes.data, None) == E_ARG  # offsets[0] != 0
    assert host(h, ids.ctypes.data, offs.ctypes.data, 1, SKIP, None, 0, oo.ctypes.data, None) == 0


# ---- 9 ------------------------------------------------------------------------------------------------------------------
VG_MARKERS = {"<|endoftext|>": 50256, "<|im_start|>": 50257}


def test_python_surface(vg_files):
    import torch

    import hutoken_amd
    vp, sp, kw = vg_files
    hutoken_amd.initialize(vp, sp, prefix=kw["prefix"], is_byte_encoder=kw["is_byte_encoder"], device=0)
    hutoken_amd.set_special_tokens(VG_MARKERS)
    rng = random.Random(39)
    marks = list(VG_MARKERS)
    texts = []
    for _ in range(200):
        pieces = [H.random_text(rng) for _ in range(rng.randint(1, 4))]
        texts.append("".join(p + rng.choice(marks + [""]) for p in pieces))
    texts += ["", marks[0], marks[1] + marks[0], "a" + marks[1] + "b", " x" + marks[0] + " y"]
    plain = [t.replace(marks[0], "").replace(marks[1], "") for t in texts]
    enc = hutoken_amd.batch_encode_special(texts)
    assert sum(e.count(50256) + e.count(50257) for e in enc) == sum(t.count("<|") for t in texts) > 100
    assert hutoken_amd.batch_decode_special(enc) == texts
    assert hutoken_amd.batch_decode_special(enc, skip_special_tokens=True) == plain
    for t, e, p in list(zip(texts, enc, plain))[-8:]:
        assert hutoken_amd.encode_special(t) == e
        assert hutoken_amd.decode_special(e) == t
        assert hutoken_amd.decode_special(e, skip_special_tokens=True) == p
    # device tensors in and out, on a stream of the caller's and on torch's default one
    data = b"".join(t.encode("utf-8") for t in texts)
    offs = np.concatenate([[0], np.cumsum([len(t.encode("utf-8")) for t in texts])]).astype(np.int64)
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    do = torch.from_numpy(offs).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        ids, oo = hutoken_amd.encode_special_packed_device(db, do)
        raw, out_oo = hutoken_amd.decode_packed_device(ids, oo, special=True)
        raw_skip, skip_oo = hutoken_amd.decode_packed_device(ids, oo, special=True, skip_special_tokens=True,
                                                             n_ids=int(oo[-1].item()))
    side.synchronize()
    assert bytes(raw.cpu().numpy()) == data and np.array_equal(out_oo.cpu().numpy(), offs)
    assert bytes(raw_skip.cpu().numpy()) == "".join(plain).encode("utf-8")
    assert skip_oo.cpu().tolist() == np.concatenate([[0], np.cumsum([len(p.encode("utf-8")) for p in plain])]).tolist()
    raw0, oo0 = hutoken_amd.decode_packed_device(ids, oo, special=True)  # (the NULL stream: through the side stream)
    torch.cuda.synchronize()
    assert torch.equal(raw0, raw) and torch.equal(oo0, out_oo)
    # special=False is the plain decode: 50256 is a vocabulary line of VG, 50257 is not
    with pytest.raises(ValueError, match="less than vocab size"):
        hutoken_amd.decode_packed_device(ids, oo)
    only_eot = [hutoken_amd.encode_special(t) for t in ("a" + marks[0] + " b", "", "c")]
    flat = torch.tensor([i for e in only_eot for i in e], dtype=torch.int32, device=dev)
    bounds = torch.tensor(np.concatenate([[0], np.cumsum([len(e) for e in only_eot])]), dtype=torch.int64, device=dev)
    raw1, oo1 = hutoken_amd.decode_packed_device(flat, bounds)
    assert bytes(raw1.cpu().numpy()).decode() == "".join(hutoken_amd.decode(e) for e in only_eot if e)
    assert oo1[-1].item() == raw1.numel() and oo1[1].item() == oo1[2].item()
    with pytest.raises(ValueError, match="special=True"):
        hutoken_amd.decode_packed_device(flat, bounds, skip_special_tokens=True)
    # the plain decode still refuses the ids the special encode makes
    with pytest.raises(ValueError, match="less than vocab size"):
        hutoken_amd.decode(hutoken_amd.encode_special("a<|im_start|>b"))
    assert hutoken_amd.decode_special(hutoken_amd.encode_special("a<|im_start|>b")) == "a<|im_start|>b"
    hutoken_amd.set_special_tokens(None)
    with pytest.raises(ValueError, match="less than vocab size"):  # no set: the plain decode
        hutoken_amd.decode_special([64, 50257])
    assert hutoken_amd.decode_special([64, 50256]) == hutoken_amd.decode([64, 50256])
