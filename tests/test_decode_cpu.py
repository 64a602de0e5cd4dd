"""tests/decode_ref.py (what the GPU decode tests compare with) against the CPU oracle, document by document: the two
long-token vocabularies and the small ones, random id lists, every added token alone, in front and behind another
token, and a sample of the tile-scale batches of tests/decode_cases.py with the sizes they are built to have."""
import random

import numpy as np
import pytest

import decode_cases as DC
import helpers as H
from decode_ref import DecodeRef


def _vocabs():
    for seed in (0, 1):
        e, s, _t = H.long_token_byte_vocab(seed)
        yield "lb%d" % seed, e, s, None, True
        yield "lbp%d" % seed, e, s, "Ġ", True
        e, s, _t = H.long_token_char_vocab(seed)
        yield "lc%d" % seed, e, s, "▁", False
    e, s = H.random_byte_vocab(3, n_merges=500, proper=False)
    yield "b3", e, s, None, True
    e, s = H.random_char_vocab(2, n_merges=500)
    yield "c2", e, s, "▁", False
    e, s = H.random_char_vocab(4, n_merges=200)
    yield "c4", e, s, None, False


def _same(orc, ref, docs, tag):
    """every document alone, the plain way; then all of them as one packed batch"""
    for ids in docs:
        want, st = orc.decode_bytes(ids)
        assert st == 0 and ref.decode_doc(ids) == (want, 0), (tag, ids[:8])
    flat, offs = DC.pack(docs)
    out, oo = ref.decode_packed(flat, offs)
    assert (ref.status(flat, offs) == 0).all()
    raw = out.tobytes()
    assert oo[0] == 0 and oo[-1] == len(raw)
    for d, ids in enumerate(docs):
        assert raw[oo[d]:oo[d + 1]] == orc.decode_bytes(ids)[0], (tag, d, ids[:8])


@pytest.mark.parametrize("name", [v[0] for v in _vocabs()])
def test_ref_against_oracle(tmp_path, oracle_mod, name):
    _n, ents, special, prefix, is_byte = next(v for v in _vocabs() if v[0] == name)
    vp, sp = H.write_vocab(tmp_path, name, ents, special)
    orc, ref = oracle_mod.Oracle(vp, sp, prefix, is_byte), DecodeRef(ents, special, prefix, is_byte)
    rng = random.Random(len(ents))
    n = len(ents)
    docs = [[rng.randrange(n) for _ in range(rng.randint(0, 12))] for _ in range(1500)] + [[], []]
    added = range(n - 40 if name[0] != "l" else (556 if is_byte else 300), n)
    for i in added:  # alone, in front of another token, behind one, twice
        docs += [[i], [i, rng.randrange(n)], [rng.randrange(n), i], [i, i]]
    _same(orc, ref, docs, name)


def test_ref_statuses(tmp_path, oracle_mod):
    """ids out of range, an id with two keys, an id with no key: the oracle's status and the reference's, per document"""
    ents, special = H.random_byte_vocab(8, n_merges=100, dup_ids=True)
    vp, sp = H.write_vocab(tmp_path, "dup", ents, special)
    orc, ref = oracle_mod.Oracle(vp, sp, None, True), DecodeRef(ents, special, None, True)
    from collections import Counter
    cnt = Counter(i for _k, i in ents)
    dup = next(i for i, c in cnt.items() if c > 1)
    hole = next(i for i in range(len(ents)) if i not in cnt)
    docs = [[1, 2], [3, dup, 4], [], [hole], [5], [len(ents)], [-1, 7], [6, 6]]
    flat, offs = DC.pack(docs)
    want = [0, 4, 0, 4, 0, 3, 3, 0]
    assert ref.status(flat, offs).tolist() == want
    assert [ref.decode_doc(d)[1] for d in docs] == want
    # (the oracle has its own numbering: 1 out of range, 2 no key, 3 two keys)
    assert [orc.decode_bytes(d)[1] for d in docs] == [0, 3, 0, 2, 0, 1, 1, 0]
    out, oo = ref.decode_packed(flat, offs)
    good = [d for d, w in zip(docs, want) if w == 0]
    assert [out[oo[k]:oo[k + 1]].tobytes() for k, w in enumerate(want) if w == 0] == [orc.decode_bytes(d)[0] for d in good]


def _tile_totals(ref, ids, offs):
    ln = ref.lengths(ids, offs)
    return np.add.reduceat(ln, np.arange(0, len(ln), DC.TILE)) if len(ln) else np.zeros(0, dtype=np.int64)


def test_tile_scale_cases(tmp_path, oracle_mod):
    """The batches of decode_cases have the sizes the GPU tests need them to have, and the reference decodes a seeded
    sample of their documents like the oracle."""
    vb, vc, vp = DC.Vocab("byte"), DC.Vocab("char"), DC.Vocab("byte", prefix="Ġ")
    orcs = {}
    for v, name in ((vb, "b"), (vc, "c"), (vp, "p")):
        paths = v.write(tmp_path, name)
        orcs[name] = oracle_mod.Oracle(*paths, v.prefix, v.is_byte)
    rng = random.Random(3)

    def sample(v, name, ids, offs, k=40):
        out, oo = v.ref.decode_packed(ids, offs)
        raw = out.tobytes()
        nd = len(offs) - 1
        for d in ([0, nd - 1] + [rng.randrange(nd) for _ in range(k)]) if nd else []:
            if offs[d + 1] - offs[d] > 2 * DC.TILE + 2:  # (the oracle takes seconds for a document of 100 k ids)
                continue
            want, st = orcs[name].decode_bytes(ids[offs[d]:offs[d + 1]])
            assert st == 0 and raw[oo[d]:oo[d + 1]] == want, (name, d)

    for case, ids, offs in DC.tile_total_cases(vb):
        assert _tile_totals(vb.ref, ids, offs)[0] == int(case[5:case.index("_")]), case
        sample(vb, "b", ids, offs)
    for case, ids, offs in DC.staging_cases(vc):
        tot = _tile_totals(vc.ref, ids, offs)
        if case[5:].isdigit():
            assert tot[0] == int(case[5:]), case
        else:
            assert tot[0] <= DC.STAGE < tot[1] and tot[2] <= DC.STAGE and tot[0] % 2 and (tot[0] + tot[1]) % 2, tot
        sample(vc, "c", ids, offs)
    for v, name in ((vc, "c"), (vb, "b")):
        for case, ids, offs in DC.inline_cases(v):
            assert set(v.ref.lengths(ids, offs).tolist()) == set(range(0 if name == "c" else 1, 9))
            sample(v, name, ids, offs)
    for v, name in ((vc, "c"), (vp, "p")):
        for case, ids, offs in DC.prefix_cases(v):
            assert set(range(32)) <= set((offs[:-1] % 32).tolist())
            assert {DC.TILE - 1, DC.TILE, 2 * DC.TILE - 1, 2 * DC.TILE} <= set(offs.tolist())
            sample(v, name, ids, offs, k=190)
    for n in (9, 2049, 65 * 2048 + 1):
        for case, ids, offs in DC.size_cases(vb, n):
            assert offs[-1] == n == len(ids)
            sample(vb, "b", ids, offs, k=10)
    tot = np.concatenate([_tile_totals(vb.ref, ids, offs) for _c, ids, offs in DC.size_cases(vb, 65 * 2048 + 1)[:1]])
    assert (tot > DC.STAGE).any() and (tot < DC.STAGE).any()  # both store paths


def test_shipped_vocabulary_case(vg_files, oracle_mod):
    """The batch of VG's long tokens has tiles on both sides of the staging threshold, next to each other both ways."""
    vp, sp, kw = vg_files
    ref = DC.shipped_vocab_ref(vg_files)
    orc = oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    ids, offs = DC.shipped_vocab_case(ref)
    tot = _tile_totals(ref, ids, offs)
    assert (tot > DC.STAGE).tolist() == [False, True, True, True, False, False], tot
    out, oo = ref.decode_packed(ids, offs)
    assert (ref.status(ids, offs) == 0).all()
    raw, rng = out.tobytes(), random.Random(4)
    for d in [0, len(offs) - 2] + [rng.randrange(len(offs) - 1) for _ in range(60)]:
        assert (raw[oo[d]:oo[d + 1]], 0) == orc.decode_bytes(ids[offs[d]:offs[d + 1]]), d
