"""tests/spans_cases.py held to its claims without a GPU: the constants are the kernels', every case hits the tile,
wavefront, lane, slot, look-back, block and chunk positions it is built for (recomputed from its arrays), its text is
what the oracle decodes its ids to, its status under tests/spans_ref.py is 0 (the tampered victims' is not), and the
numpy form of the reference that tests/test_gpu_spans_edges.py compares with equals spans_ref.batch element for element."""
import numpy as np
import pytest

import spans_cases as SC
import spans_ref as S
import view_cases as V

PAIRS = [(f, k) for f in SC.FAMILIES for k in SC.KINDS if SC.applies(f, k)]


@pytest.fixture(scope="module")
def oracles(tmp_path_factory, oracle_mod):
    tmp = tmp_path_factory.mktemp("spans_cases")
    out = {}
    for kind in SC.KINDS:
        v = SC.vocab(kind)
        vp, sp = v.write(tmp, kind)
        out[kind] = oracle_mod.Oracle(vp, sp, v.prefix, v.is_byte)
    return out


def test_constants_are_the_kernels():
    from hutoken_amd import _capi
    lib = _capi.load()
    assert SC.SP_TILE == lib.hutk_debug_span_tile_ids() == SC.SP_THREADS * SC.SP_PER
    assert SC.SPAN_CHUNK_BYTES == lib.hutk_debug_span_chunk_bytes() == V.SPAN_CHUNK_BYTES
    assert SC.SP_PER == V.SP_PER and SC.SP_THREADS % SC.WAVE == 0 and SC.SPAN_CHUNK_BYTES % SC.BLOCK == 0


def test_vocabularies_hold_what_the_families_need():
    b, c = SC.vocab("byte"), SC.vocab("char")
    assert sorted(bytes(b.ref.blob[b.ref.off[i]:b.ref.off[i] + 1]) for i in range(256)) == [bytes([x]) for x in range(256)]
    assert set(range(2, 9)) <= set(b.ref.len[:b.n_base].tolist()) and {13, 600} <= set(b.ref.len.tolist())
    assert not (b.ref.slen != b.ref.len).any()  # no prefix: nothing differs at a document's front
    for ch in SC.UNKNOWN_ITEMS:
        assert ch.decode("utf-8") not in c.id and not any(ch.decode("utf-8") in t for t in c.tokens)
    assert [len(ch) for ch in SC.UNKNOWN_ITEMS] == [1, 2, 3, 4]
    empty_first = [i for i in range(c.ref.n) if c.ref.slen[i] == 0]
    assert empty_first == [c.id["▁"]] and not (c.ref.len == 0).any()
    assert len(SC.first_differs(c)) == 25
    assert sorted(SC.width_ids(c)) == [5, 6, 7, 8, 9, 10] and sorted(SC.width_ids(b)) == [5, 6, 7, 8, 13, 26]
    for L, i in SC.width_ids(c).items():
        assert (c.ref.blob[c.ref.off[i]:c.ref.off[i] + L] >= 0x80).any()


@pytest.mark.parametrize("kind", SC.KINDS)
def test_ref_text_is_the_oracles_token_text(oracles, kind):
    v = SC.vocab(kind)
    mine, theirs = SC.RefText(v.ref), S.TokenText(oracles[kind])
    for i in range(v.ref.n):
        assert mine.first(i) == theirs.first(i) and mine.rest(i) == theirs.rest(i), (kind, i, v.tokens[i])
    assert mine.first(-1) is None and mine.rest(v.ref.n) is None


def _pin(v, c, kind):
    """spans_ref.batch, unchanged, against the numpy form: every element, both units"""
    tt = SC.RefText(v.ref)
    for unit in ("byte", "char"):
        want, st = S.batch(tt, c.data, c.offsets, c.ids, c.id_offsets, v.is_byte, unit, np.int64)
        assert not st.any(), (c.name, unit, np.nonzero(st)[0][:5])
        got = SC.want(kind, c, unit)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (c.name, unit, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("family,kind", PAIRS)
def test_every_case_keeps_its_claims(oracles, family, kind):
    v, orc = SC.vocab(kind), oracles[kind]
    cases = SC.cases(family, kind)
    assert cases and len({c.name for c in cases}) == len(cases)
    for c in cases:
        n_docs = len(c.offsets) - 1
        assert c.data.dtype == np.uint8 and c.ids.dtype == np.int32 and c.offsets.dtype == c.id_offsets.dtype == np.int64
        assert len(c.id_offsets) == n_docs + 1 and c.offsets[0] == 0 and c.id_offsets[0] == 0
        assert c.offsets[-1] == len(c.data) and c.id_offsets[-1] == len(c.ids)
        m = SC.measure(v, c)
        assert SC.holds(c.claims, m) is None, (c.name, SC.holds(c.claims, m))
        for p in c.claims.get("cont", []):
            assert (c.data[p] & 0xC0) == 0x80 and (c.data[p - 1] & 0xC0) != 0x80, (c.name, p)
        raw = c.data.tobytes()
        if kind == "char":
            assert raw.decode("utf-8").encode("utf-8") == raw, c.name  # well-formed: that mode's contract
        for d in range(n_docs):  # the text is the oracle's decoding of the ids
            ids = c.ids[int(c.id_offsets[d]):int(c.id_offsets[d + 1])]
            if not (ids == -1).any():
                out, st = orc.decode_bytes(ids)
                assert st == 0 and out == raw[int(c.offsets[d]):int(c.offsets[d + 1])], (c.name, d)
        _pin(v, c, kind)
        print("%s %s: %d docs, %d ids, %d bytes" % (kind, c.name, n_docs, len(c.ids), len(c.data)))


def _all(kind):
    return [(c, SC.measure(SC.vocab(kind), c)) for f in SC.FAMILIES for c in SC.cases(f, kind)]


@pytest.mark.parametrize("kind", SC.KINDS)
def test_the_families_reach_what_the_kernels_branch_on(kind):
    got = _all(kind)
    starts = set().union(*(m["starts"] for _c, m in got))
    empties = set().union(*(m["empty_at"] for _c, m in got))
    for t in SC.START_TILES:
        for w in range(SC.SP_THREADS // SC.WAVE):
            for lane in SC.START_LANES:
                for k in range(SC.SP_PER):
                    assert (t, w, lane, k) in starts and (t, w, lane, k) in empties, (t, w, lane, k)
    assert SC.DEPTHS <= set().union(*(m["depths"] for _c, m in got)) and max(max(m["depths"], default=0) for _c, m in got) >= 128
    assert max(m["tile_starts"] for _c, m in got) == SC.SP_TILE
    assert max(m["empty_run"] for _c, m in got) > SC.SP_THREADS
    for key, mod in (("ends", SC.BLOCK), ("bases", SC.BLOCK), ("ends", SC.SPAN_CHUNK_BYTES), ("bases", SC.SPAN_CHUNK_BYTES)):
        hit = set().union(*(m["%s%d" % (key, mod)] for _c, m in got))
        assert {0, 1, mod - 1} <= hit, (key, mod)
    assert set(SC.N_BYTES) | {1, 7, 15, 16, 17} | ({0} if kind == "char" else set()) <= {m["n_bytes"] for _c, m in got}
    assert set(SC.SIZES) <= {m["n_ids"] for _c, m in got}
    if kind == "byte":
        assert max(m["cont_blocks"] for _c, m in got) >= 2
    unknown = [c for c, _m in got if (c.ids == -1).any()]
    assert len(unknown) >= 4 and max(int((c.ids == -1).sum()) for c in unknown) >= 2100


def test_the_claims_are_no_formality():
    """the same batches moved by one token or one byte do not keep them"""
    v = SC.vocab("byte")
    c = SC.cases("start_position", "byte")[0]
    moved = SC.assemble(v, "moved", c.ids[1:], np.maximum(c.id_offsets - 1, 0))
    assert SC.holds(c.claims, SC.measure(v, moved)) is not None
    c = SC.cases("size", "byte")[-1]
    short = SC.assemble(v, "short", c.ids[:-SC.SP_TILE], np.minimum(c.id_offsets, len(c.ids) - SC.SP_TILE))
    assert SC.holds(c.claims, SC.measure(v, short)) is not None
    c = next(x for x in SC.cases("rank_edge", "byte") if x.name.endswith("ends_and_bases_on_the_edges"))
    pad = SC.assemble(v, "pad", np.concatenate([c.ids[:1], c.ids[:1], c.ids]),
                      np.concatenate([[0], c.id_offsets[1:] + 2]))
    assert SC.holds(c.claims, SC.measure(v, pad)) is not None


@pytest.mark.parametrize("kind", SC.KINDS)
def test_a_tampered_victim_is_the_references_only_mismatch(kind):
    v = SC.vocab(kind)
    tampered = SC.tamper_cases(v)
    assert len(tampered) == 3
    tt = SC.RefText(v.ref)
    for c, victim, bad, st in tampered:
        at = np.nonzero(bad != c.ids)[0]
        assert len(at) == 1 and c.id_offsets[victim] <= at[0] < c.id_offsets[victim + 1]
        a, b = int(c.ids[at[0]]), int(bad[at[0]])
        first = at[0] == c.id_offsets[victim]
        ta, tb = (tt.first(a), tt.first(b)) if first else (tt.rest(a), tt.rest(b))
        assert ta[:1] != tb[:1] and len(ta) != len(tb)
        assert st[victim] == S.MISMATCH and int((st != 0).sum()) == 1, c.name
        assert SC.holds(c.claims, SC.measure(v, c)) is None
        _pin(v, c, kind)
    c, victim, _bad, _st = tampered[0]
    assert c.id_offsets[victim + 1] == SC.SP_TILE
    c, victim, _bad, _st = tampered[1]
    assert c.id_offsets[victim + 1] - c.id_offsets[victim] >= 3 * SC.SP_TILE
    c, victim, _bad, _st = tampered[2]
    assert SC.measure(v, c)["tile_starts"] == SC.SP_TILE and c.id_offsets[victim + 1] - c.id_offsets[victim] == 1
