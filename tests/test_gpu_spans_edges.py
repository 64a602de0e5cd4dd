"""The span kernels (hutk_spans.hip) on batches of ids built by their own constants (tests/spans_cases.py): document
starts on every slot, lane and wavefront of a tile, tiles that are all starts, look-back over one, two and three
windows, tokens without text, decode-table entries around the inline width, token ends and document bases on the edges
of the rank structure's blocks and chunks, ids of -1 placed on purpose, a tampered id at the tile edges, and one context
on large, tiny and empty batches in turn.

Every case goes through Context.token_spans_packed in both units and both widths, and EVERY element is compared with
the reference (spans_cases.expected, which tests/test_spans_cases_cpu.py holds equal to spans_ref.batch on every case);
under HUTK_SPANS_HELP_AFTER=0 and HUTK_SPANS_SELECT=search the results are compared with that reference too, not with the
default run.  Needs a real MI355X."""
import numpy as np
import pytest

import spans_cases as SC
import spans_ref as S

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = 6
UNITS = (("byte", 0), ("char", 1))
WIDTHS = ((4, np.int32), (8, np.int64))


@pytest.fixture(scope="module")
def ctxs(tmp_path_factory):
    from hutoken_amd import _capi
    assert _capi.load().hutk_debug_span_tile_ids() == SC.SP_TILE
    assert _capi.load().hutk_debug_span_chunk_bytes() == SC.SPAN_CHUNK_BYTES
    tmp = tmp_path_factory.mktemp("spans_edges")
    out = {}
    for kind in SC.KINDS:
        v = SC.vocab(kind)
        vp, sp = v.write(tmp, kind)
        out[kind] = _capi.Context(vp, sp, v.prefix, v.is_byte, device=0)
    yield out
    for ctx in out.values():
        ctx.close()


def check(ctx, kind, c, tag=""):
    """one case, both units, both widths: rc 0, no status, every element"""
    n_tiles = (len(c.ids) + SC.SP_TILE - 1) // SC.SP_TILE
    print("%s %s%s: %d docs, %d ids, %d tiles, %d bytes" % (kind, c.name, tag, len(c.offsets) - 1, len(c.ids), n_tiles, len(c.data)))
    for unit, code in UNITS:
        want = SC.want(kind, c, unit)
        for width, dtype in WIDTHS:
            got, st, rc = ctx.token_spans_packed(c.data, c.offsets, c.ids, c.id_offsets, unit=code, out_width=width)
            where = (kind, c.name + tag, unit, width)
            assert rc == 0 and not st.any(), (where, rc, np.nonzero(st)[0][:5])
            assert got.dtype == dtype and got.shape == want.shape, where
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (where, "%d rows differ, the first at" % bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_family(ctxs, family):
    for kind in SC.KINDS:
        for c in SC.cases(family, kind):
            check(ctxs[kind], kind, c)


@pytest.mark.parametrize("family", ["size", "start_position"])
def test_family_when_every_tile_helps_itself(ctxs, monkeypatch, family):
    """HUTK_SPANS_HELP_AFTER=0: a tile adds an unanswered predecessor up itself at its first poll"""
    monkeypatch.setenv("HUTK_SPANS_HELP_AFTER", "0")
    for kind in SC.KINDS:
        for c in SC.cases(family, kind):
            check(ctxs[kind], kind, c, " help_after=0")


@pytest.mark.parametrize("family", SC.FAMILIES)
def test_family_with_select_by_search(ctxs, monkeypatch, family):
    """HUTK_SPANS_SELECT=search: character mode without the scattered select array"""
    monkeypatch.setenv("HUTK_SPANS_SELECT", "search")
    for c in SC.cases(family, "char"):
        check(ctxs["char"], "char", c, " select=search")


@pytest.mark.parametrize("kind", SC.KINDS)
def test_a_tampered_id_at_the_tile_edges_marks_its_document_only(ctxs, kind):
    ctx = ctxs[kind]
    for c, victim, bad_ids, ref_status in SC.tamper_cases(SC.vocab(kind)):
        assert ref_status[victim] == S.MISMATCH and int((ref_status != 0).sum()) == 1
        a, b = int(c.id_offsets[victim]), int(c.id_offsets[victim + 1])
        print("%s %s: %d docs, %d ids, victim %d = ids [%d, %d)" % (kind, c.name, len(c.offsets) - 1, len(c.ids), victim, a, b))
        for unit, code in UNITS:
            want = SC.want(kind, c, unit)
            for width, _dtype in WIDTHS:
                got, st, rc = ctx.token_spans_packed(c.data, c.offsets, bad_ids, c.id_offsets, unit=code, out_width=width)
                where = (kind, c.name, unit, width)
                assert rc == E_UNSUPPORTED, where
                assert np.array_equal(st, ref_status), (where, np.nonzero(st != ref_status)[0][:5])
                others = np.ones(len(c.ids), dtype=bool)
                others[a:b] = False
                wrong = np.nonzero(((got != want).any(axis=1)) & others)[0]
                assert wrong.size == 0, (where, wrong[:5], got[wrong[:5]], want[wrong[:5]])


def test_one_context_on_large_tiny_empty_and_large_batches(ctxs):
    """The workspace (first-token bits, tile states, rank arrays, the select table) stays between calls and is cleared
    only as far as each call needs: 129 tiles, one id, documents without ids, four tiles, 129 tiles again -- in character
    mode, where the select table is kept."""
    ctx, kind = ctxs["char"], "char"
    v = SC.vocab(kind)
    big = SC.cases("size", kind)[-1]
    one = SC.cases("size", kind)[0]
    assert len(big.ids) == SC.SIZES[-1] and len(one.ids) == 1
    nothing = SC.assemble(v, "reuse/300_documents_without_ids", [], np.zeros(301, dtype=np.int64))
    for c in (big, one, nothing, SC.cases("start_position", kind)[0], big):
        check(ctx, kind, c, " (reuse)")
