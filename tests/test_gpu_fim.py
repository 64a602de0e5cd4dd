"""Fill-in-the-middle on the GPU (hutk_fim_cut_text_device, hutk_fim_plan_tokens_device, hutk_fim_plan_pieces_device,
hutk_fim_render_device, fim_device, fim_cut_text_device, fim_pieces_device, batch_encode_fim) against fim_ref, element by
element in every output with a sentinel-filled guard behind each, on the smallest shapes at which the kernels can go
wrong: the edges of a workgroup's span, a document longer than several spans, thousands of empty documents at one place,
over a thousand documents in one span, the blocks of the scan, forced cuts, the rates, views off the 16-byte boundary,
inputs the range checks must reject, the text cut on every continuation byte, and the composition with encode,
collation, packing and the token spans."""
import random

import numpy as np
import pytest

import fim_ref as R
import packed_ref
from hutoken_amd import _capi

pytestmark = pytest.mark.gpu

IGN = -100
GUARD = 64
SENT32, SENT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
NO = _capi.NO_TOKEN
ONE = 2**32
PRE, SUF, MID, END = 60001, 60002, 60003, 60004
PER_TOKEN = ("out_ids", "labels", "parts", "source")
S = None


@pytest.fixture(scope="module", autouse=True)
def span():
    global S
    S = _capi.fim_span()
    assert S >= 64
    return S


def _dev(values, dtype, off=0):
    """values on the GPU as a view `off` elements behind a 16-byte boundary"""
    import torch
    arr = np.asarray(values, dtype=dtype)
    base = torch.zeros(arr.size + off + 4, dtype=getattr(torch, np.dtype(dtype).name), device="cuda:0")
    view = base[off:off + arr.size]
    view.copy_(torch.from_numpy(arr))
    assert arr.size == 0 or view.data_ptr() % 16 == (off * arr.itemsize) % 16
    return view


def _outputs(cap, off, only_ids=False):
    outs = {"out_ids": _dev(np.full(cap + GUARD, SENT32), np.int32, off)}
    if not only_ids:
        outs["labels"] = _dev(np.full(cap + GUARD, SENT32), np.int32, off)
        outs["parts"] = _dev(np.full(cap + GUARD, SENT32), np.int32, off)
        outs["source"] = _dev(np.full(cap + GUARD, SENT64), np.int64, off)
    return outs


def _render(d_ids, plan, kinds, oo, n_docs, n_ids, end, loss, cap, outs, d_err):
    ptr = lambda k: outs[k].data_ptr() if k in outs else 0  # noqa: E731
    _capi.fim_render_device(d_ids.data_ptr(), plan.data_ptr(), kinds.data_ptr(), oo.data_ptr(), n_docs, n_ids, PRE, SUF, MID,
                            NO if end is None else end, loss, IGN, cap, ptr("out_ids"), ptr("labels"), ptr("parts"), ptr("source"),
                            d_err, 0)


def _finish(outs, plan, kinds, oo, err, cap, n_docs):
    import torch
    try:
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in outs.items()}
        res.update(plan=plan.cpu().numpy().reshape(-1, 4)[:n_docs], kinds=kinds.cpu().numpy()[:n_docs], out_offsets=oo.cpu().numpy(),
                   err=err.cpu().numpy().tolist(), cap=cap)
    except RuntimeError as ex:
        pytest.exit("device failure, nothing more is run: %s" % ex, returncode=3)
    return res


def run_tokens(ids, offsets, *, seed, fb, sb, first=0, end=END, loss=R.LOSS_ALL, off=0, out_cap=None, n_ids=None, only_ids=False):
    """plan (tokens) and render on fresh, sentinel-filled outputs with a guard behind the capacity.  off = 1: every buffer
    is a view one element off the 16-byte boundary."""
    n_docs = len(offsets) - 1
    n_ids = len(ids) if n_ids is None else n_ids
    cap = _capi.fim_ids_bound(n_docs, n_ids, end is not None) if out_cap is None else out_cap
    d_ids, d_offs = _dev(ids, np.int32, off), _dev(offsets, np.int64, off)
    oo = _dev([SENT64] * (n_docs + 1), np.int64, off)
    plan, kinds = _dev([SENT64] * (4 * n_docs + 4), np.int64, off), _dev([SENT32] * (n_docs + 1), np.int32, off)
    outs, err = _outputs(cap, off, only_ids), _dev([-7, -7], np.int32, off)
    _capi.fim_plan_tokens_device(d_offs.data_ptr(), n_docs, n_ids, seed, first, fb, sb, end is not None, oo.data_ptr(),
                                 plan.data_ptr(), kinds.data_ptr(), err[0:].data_ptr(), 0)
    _render(d_ids, plan, kinds, oo, n_docs, n_ids, end, loss, cap, outs, err[1:].data_ptr())
    return _finish(outs, plan, kinds, oo, err, cap, n_docs)


def run_pieces(ids, piece_offsets, kinds, *, end=END, loss=R.LOSS_ALL, off=0, out_cap=None):
    n_docs = (len(piece_offsets) - 1) // 3
    cap = _capi.fim_ids_bound(n_docs, len(ids), end is not None) if out_cap is None else out_cap
    d_ids, d_offs = _dev(ids, np.int32, off), _dev(piece_offsets, np.int64, off)
    d_kinds = _dev(list(kinds) + [SENT32], np.int32, off)
    oo, plan = _dev([SENT64] * (n_docs + 1), np.int64, off), _dev([SENT64] * (4 * n_docs + 4), np.int64, off)
    outs, err = _outputs(cap, off), _dev([-7, -7], np.int32, off)
    _capi.fim_plan_pieces_device(d_offs.data_ptr(), d_kinds.data_ptr(), n_docs, len(ids), end is not None, oo.data_ptr(),
                                 plan.data_ptr(), err[0:].data_ptr(), 0)
    _render(d_ids, plan, d_kinds, oo, n_docs, len(ids), end, loss, cap, outs, err[1:].data_ptr())
    return _finish(outs, plan, d_kinds, oo, err, cap, n_docs)


def run_render(ids, plan, kinds, oo, *, end=END, loss=R.LOSS_ALL, out_cap=None, n_ids=None):
    """the render alone, on a plan, kinds and out_offsets of the caller's"""
    n_docs = len(kinds)
    n_ids = len(ids) if n_ids is None else n_ids
    cap = _capi.fim_ids_bound(n_docs, n_ids, end is not None) if out_cap is None else out_cap
    d_ids, d_plan = _dev(ids, np.int32), _dev(np.asarray(plan).reshape(-1), np.int64)
    d_kinds, d_oo = _dev(kinds, np.int32), _dev(oo, np.int64)
    outs, err = _outputs(cap, 0), _dev([0, -7], np.int32)
    _render(d_ids, d_plan, d_kinds, d_oo, n_docs, n_ids, end, loss, cap, outs, err[1:].data_ptr())
    return _finish(outs, d_plan, d_kinds, d_oo, err, cap, n_docs)


def assert_guard(got, n_written):
    """nothing is written at or behind `n_written` (the sequences' end, or the capacity)"""
    for k in PER_TOKEN:
        if k in got:
            tail = got[k][n_written:]
            assert (tail == (SENT64 if k == "source" else SENT32)).all(), "%s was written behind element %d" % (k, n_written)


def assert_equal(got, want, want_err=0):
    assert max(got["err"]) == want_err, got["err"]
    assert np.array_equal(got["out_offsets"], want["out_offsets"])
    n_out = len(want["out_ids"])
    assert n_out <= got["cap"]
    for k in PER_TOKEN:
        if k in got:
            bad = np.nonzero(got[k][:n_out] != want[k])[0]
            assert bad.size == 0, "%s differs at %d of %d: got %d, want %d" % (k, bad[0], n_out, got[k][bad[0]], want[k][bad[0]])
    assert_guard(got, n_out)


def check_tokens(ids, offsets, *, seed, fb, sb, first=0, end=END, loss=R.LOSS_ALL, **kw):
    want = R.fim_tokens(ids, offsets, seed=seed, fim_below=fb, spm_below=sb, first_doc=first, pre=PRE, suf=SUF, mid=MID, end=end,
                        loss_parts=loss, ignore_index=IGN)
    got = run_tokens(ids, offsets, seed=seed, fb=fb, sb=sb, first=first, end=end, loss=loss, **kw)
    assert np.array_equal(got["plan"], want["plan"]) and np.array_equal(got["kinds"], want["kinds"])
    assert_equal(got, want)
    return got, want


class Forced:
    """documents with cuts and kinds of the test's choosing, as the pieces entry point takes them"""

    def __init__(self, seed=0):
        self.rng = random.Random(seed)
        self.ids, self.offsets, self.kinds = [], [0], []

    def doc(self, n, lo=None, hi=None, kind=R.PLAIN):
        lo, hi = (n, n) if lo is None else (lo, hi)
        assert 0 <= lo <= hi <= n
        base = len(self.ids)
        self.ids += [self.rng.randrange(1000, 50000) for _ in range(n)]
        self.offsets += [base + lo, base + hi, base + n]
        self.kinds.append(kind)
        return self

    def rendered(self, E=1):
        return sum(R.rendered_length(o1 - o0, k, E) for o0, o1, k in zip(self.offsets[0::3], self.offsets[3::3], self.kinds))

    def check(self, end=END, loss=R.LOSS_ALL, **kw):
        want = R.render(self.ids, R.plan_pieces(self.offsets), self.kinds, pre=PRE, suf=SUF, mid=MID, end=end, loss_parts=loss,
                        ignore_index=IGN)
        got = run_pieces(self.ids, self.offsets, self.kinds, end=end, loss=loss, **kw)
        assert np.array_equal(got["plan"], R.plan_pieces(self.offsets))
        assert_equal(got, want)
        return got, want


def ragged(rng, lengths):
    offsets = np.cumsum([0] + list(lengths)).astype(np.int64)
    return np.array([rng.randrange(1000, 50000) for _ in range(offsets[-1])], dtype=np.int32), offsets


# ---- the span's edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_documents_that_end_at_a_span_edge(lead):
    for kind in (R.PSM, R.SPM):
        for E in (0, 1):
            b = Forced(lead)
            for _ in range(lead):
                b.doc(1)
            for length in (S - 1, S, S + 1, 2 * S):
                n = length - 3 - E
                lo = b.rng.randrange(0, n + 1)
                b.doc(n, lo, b.rng.randrange(lo, n + 1), kind)
                b.doc(1)
            b.check(end=END if E else None)


def test_every_part_on_both_sides_of_a_span_edge():
    """pre, suf, mid, end and the first and the last token of prefix, middle and suffix, each once as the last position of
    a span and once as the first of the next: a plain document in front puts it there."""
    P, M, X = 5, 6, 7  # the parts' lengths (X: the suffix)
    n = P + M + X
    for kind in (R.PSM, R.SPM):
        b = Forced(kind)
        layout = R.layout(n, P, P + M, kind, 1)
        marks = [q for q, (part, v) in enumerate(layout) if part == R.PART_SENTINEL or v in (0, P - 1, P, P + M - 1, P + M, n - 1)]
        assert len(marks) == 4 + 6
        for q in marks:
            for side in (S - 1, S):  # where position q of the document lands inside its span
                at = b.rendered()
                b.doc((side - q - at) % S + S)
                assert (b.rendered() + q) % S == side % S
                b.doc(n, P, P + M, kind)
        got, want = b.check()
        edges = set(np.arange(S - 1, len(want["out_ids"]), S).tolist()) | set(np.arange(S, len(want["out_ids"]), S).tolist())
        assert {int(p) for p in want["parts"][sorted(edges)]} == {0, 1, 2, 3, 4}


def test_one_long_document():
    n = 3 * S + 5
    for kind, lo, hi in ((R.PSM, S + 3, 2 * S + 1), (R.SPM, 7, 3 * S), (R.PLAIN, n, n), (R.SPM, 0, n), (R.PSM, n, n)):
        Forced(1).doc(n, lo, hi, kind).check()
    rng = random.Random(5)
    ids, offsets = ragged(rng, [n])
    check_tokens(ids, offsets, seed=3, fb=ONE, sb=ONE // 2)


def test_thousands_of_empty_documents_in_a_row():
    rng = random.Random(6)
    ids, offsets = ragged(rng, [40] + [0] * 5000 + [S + 9] + [0] * 5000 + [3] + [0] * 300)
    got, want = check_tokens(ids, offsets, seed=11, fb=ONE, sb=ONE // 2)
    assert (want["kinds"][1:5001] == R.PLAIN).all() and want["kinds"][0] != R.PLAIN  # (an empty document is never transformed)
    check_tokens(ids, offsets, seed=11, fb=ONE, sb=ONE // 2, end=None, off=1)
    # transformed empty documents (the pieces entry point allows them): sentinels only
    b = Forced(2)
    for k in range(700):
        b.doc(0, 0, 0, (R.PSM, R.SPM, R.PLAIN)[k % 3])
    b.check()
    b.check(end=None)


def test_more_than_a_thousand_documents_in_one_span():
    rng = random.Random(7)
    ids, offsets = ragged(rng, [1] * 1500 + [2] * 900)
    got, want = check_tokens(ids, offsets, seed=1, fb=0, sb=0)                     # plain: 1500 starts in the first span
    assert want["out_offsets"][1200] < S
    check_tokens(ids, offsets, seed=1, fb=ONE // 2, sb=ONE // 2)
    check_tokens(ids, offsets, seed=2, fb=ONE, sb=ONE // 2, end=None)


@pytest.mark.parametrize("n_docs", [255, 256, 257, 1000])
def test_scan_edges(n_docs):
    rng = random.Random(n_docs)
    ids, offsets = ragged(rng, [rng.choice((0, 1, 2, 5, 17, 60)) for _ in range(n_docs)])
    check_tokens(ids, offsets, seed=n_docs, fb=ONE // 2, sb=ONE // 2)
    b = Forced(n_docs)
    for _ in range(n_docs):
        n = rng.choice((0, 1, 2, 5, 17))
        lo = rng.randrange(0, n + 1)
        b.doc(n, lo, rng.randrange(lo, n + 1), rng.choice((R.PLAIN, R.PSM, R.SPM)))
    b.check()


def test_forced_cuts():
    for kind in (R.PSM, R.SPM):
        for E in (0, 1):
            b = Forced(kind)
            for n in (1, 2, 9, S):
                for lo, hi in ((0, 0), (0, n), (n, n), (0, 1), (n - 1, n), (n // 2, n // 2)):
                    b.doc(n, lo, hi, kind)
            got, want = b.check(end=END if E else None)
            assert (want["parts"] == R.PART_MIDDLE).any() and (want["parts"] == R.PART_PREFIX).any()


# ---- the rates, the losses, determinism ------------------------------------------------------------------------------------
def _mixed(seed, n_docs=600):
    rng = random.Random(seed)
    return ragged(rng, [rng.choice((0, 1, 2, 3, 8, 30, 200)) for _ in range(n_docs)])


def test_rates():
    ids, offsets = _mixed(1)
    got, want = check_tokens(ids, offsets, seed=5, fb=0, sb=ONE // 2)
    n = len(ids)
    assert np.array_equal(got["out_ids"][:n], ids) and np.array_equal(got["out_offsets"], offsets)     # bit-equal to the input
    assert (got["parts"][:n] == 0).all() and np.array_equal(got["source"][:n], np.arange(n))
    nonempty = np.diff(offsets) > 0
    for end in (END, None):
        got, want = check_tokens(ids, offsets, seed=5, fb=ONE, sb=0, end=end)
        assert (want["kinds"][nonempty] == R.PSM).all() and (want["kinds"][~nonempty] == R.PLAIN).all()
        got, want = check_tokens(ids, offsets, seed=5, fb=ONE, sb=ONE, end=end)
        assert (want["kinds"][nonempty] == R.SPM).all()
        got, want = check_tokens(ids, offsets, seed=5, fb=ONE // 2, sb=ONE // 2, end=end)
        assert set(want["kinds"].tolist()) == {0, 1, 2}
        assert ((want["out_ids"] == END).sum() > 0) == (end is not None)


@pytest.mark.parametrize("loss", [R.LOSS_ALL, R.LOSS_MIDDLE, 0, 1, 2, 4, 8, 16, 32, 0b1010, 63])
def test_every_loss(loss):
    ids, offsets = _mixed(2, 200)
    got, want = check_tokens(ids, offsets, seed=9, fb=ONE * 3 // 4, sb=ONE // 2, loss=loss)
    if loss == R.LOSS_MIDDLE:
        on = want["labels"] != IGN
        assert (on == ((want["parts"] == R.PART_MIDDLE) | (want["parts"] == R.PART_PLAIN) | (want["out_ids"] == END))).all()


def test_python_loss_on_and_outputs():
    import torch
    import hutoken_amd as H
    ids, offsets = _mixed(3, 300)
    d_ids, d_offs = torch.from_numpy(ids).cuda(), torch.from_numpy(offsets).cuda()
    sent = dict(prefix_id=PRE, suffix_id=SUF, middle_id=MID)
    for loss_on, bits in (("all", R.LOSS_ALL), ("middle", R.LOSS_MIDDLE), (("prefix", "suffix"), 0b1010), (("sentinel",), 16), ((), 0)):
        for end in (END, None):
            want = R.fim_tokens(ids, offsets, seed=77, fim_below=int(0.6 * ONE), spm_below=int(0.3 * ONE), first_doc=10, pre=PRE,
                                suf=SUF, mid=MID, end=end, loss_parts=bits, ignore_index=-1)
            out_ids, oo, labels, parts, source = H.fim_device(d_ids, d_offs, seed=77, fim_rate=0.6, spm_rate=0.3, first_doc=10,
                                                              end_id=end, loss_on=loss_on, ignore_index=-1, return_labels=True,
                                                              return_parts=True, return_source=True, check=True, **sent)
            n = len(want["out_ids"])
            assert out_ids.numel() == _capi.fim_ids_bound(len(offsets) - 1, len(ids), end is not None) >= n
            assert np.array_equal(oo.cpu().numpy(), want["out_offsets"])
            for t, k in ((out_ids, "out_ids"), (labels, "labels"), (parts, "parts"), (source, "source")):
                assert np.array_equal(t[:n].cpu().numpy(), want[k]), k
    res = H.fim_device(d_ids, d_offs, seed=77, n_ids=len(ids), return_source=True, **sent)
    assert len(res) == 3 and res[2].dtype == torch.int64
    assert len(H.fim_device(d_ids, d_offs, seed=77, **sent)) == 2
    with pytest.raises(ValueError, match="device-side error"):
        H.fim_device(d_ids, torch.flip(d_offs, [0]).contiguous(), seed=1, n_ids=len(ids), check=True, **sent)
    # no documents at all
    out_ids, oo = H.fim_device(d_ids[:0], d_offs[:1], seed=1, **sent)
    assert oo.tolist() == [0]


def test_a_batch_equals_its_halves():
    ids, offsets = _mixed(4, 500)
    whole, _ = check_tokens(ids, offsets, seed=21, fb=ONE // 2, sb=ONE // 2, first=1000)
    h = 250
    a, _ = check_tokens(ids[:offsets[h]], offsets[:h + 1], seed=21, fb=ONE // 2, sb=ONE // 2, first=1000)
    b, _ = check_tokens(ids[offsets[h]:], offsets[h:] - offsets[h], seed=21, fb=ONE // 2, sb=ONE // 2, first=1000 + h)
    na, nb = a["out_offsets"][-1], b["out_offsets"][-1]
    assert na + nb == whole["out_offsets"][-1]
    for k in ("out_ids", "labels", "parts"):
        assert np.array_equal(np.concatenate([a[k][:na], b[k][:nb]]), whole[k][:na + nb])
    assert np.array_equal(np.concatenate([a["source"][:na], np.where(b["source"][:nb] >= 0, b["source"][:nb] + offsets[h], -1)]),
                          whole["source"][:na + nb])
    assert np.array_equal(np.concatenate([a["kinds"], b["kinds"]]), whole["kinds"])
    other, _ = check_tokens(ids, offsets, seed=22, fb=ONE // 2, sb=ONE // 2, first=1000)
    assert not np.array_equal(other["kinds"], whole["kinds"])
    moved, _ = check_tokens(ids, offsets, seed=21, fb=ONE // 2, sb=ONE // 2, first=2**33)   # a document number above 2^32
    assert not np.array_equal(moved["kinds"], whole["kinds"])


def test_views_off_the_16_byte_boundary():
    ids, offsets = _mixed(5, 300)
    for end in (END, None):
        aligned, _ = check_tokens(ids, offsets, seed=4, fb=ONE // 2, sb=ONE // 2, end=end)
        shifted, _ = check_tokens(ids, offsets, seed=4, fb=ONE // 2, sb=ONE // 2, end=end, off=1)
        n = aligned["out_offsets"][-1]
        for k in PER_TOKEN:
            assert np.array_equal(aligned[k][:n], shifted[k][:n])
    got = run_tokens(ids, offsets, seed=4, fb=ONE // 2, sb=ONE // 2, end=None, off=1, only_ids=True)   # no optional output at all
    assert got["err"] == [0, 0] and np.array_equal(got["out_ids"][:n], aligned["out_ids"][:n])
    assert_guard(got, n)
    b = Forced(3)
    for k in range(40):
        b.doc(k, k // 3, k // 2, (R.PSM, R.SPM, R.PLAIN)[k % 3])
    b.check(off=1)


# ---- hostile inputs: reported, and nothing is written past the guard ----------------------------------------------------------
@pytest.mark.parametrize("case", ["decreasing", "past_the_ids", "end_is_not_n_ids", "start_is_not_0", "negative"])
def test_offsets_that_do_not_fit_are_reported(case):
    ids, offsets = _mixed(6, 300)
    offsets = offsets.copy()
    n_ids = len(ids)
    if case == "decreasing":
        offsets[100] = offsets[99] - 5
    elif case == "past_the_ids":
        offsets[100:] += 2 * n_ids
    elif case == "end_is_not_n_ids":
        n_ids -= 3
    elif case == "start_is_not_0":
        offsets[0] = 1
    else:
        offsets[50] = -4
    got = run_tokens(ids, offsets, seed=1, fb=ONE // 2, sb=ONE // 2, n_ids=n_ids)
    assert got["err"][0] == _capi.E_ARG
    assert_guard(got, got["cap"])
    assert 0 <= got["out_offsets"][-1] and (np.diff(got["out_offsets"]) >= 0).all()
    src = got["source"][:min(got["cap"], got["out_offsets"][-1])]
    assert ((src >= -1) & (src < n_ids)).all()


def _valid(seed=7, n_docs=120):
    ids, offsets = _mixed(seed, n_docs)
    want = R.fim_tokens(ids, offsets, seed=3, fim_below=ONE * 3 // 4, spm_below=ONE // 2, pre=PRE, suf=SUF, mid=MID, end=END,
                        ignore_index=IGN)
    return ids, want


@pytest.mark.parametrize("case", ["lo_above_hi", "hi_above_n", "past_the_ids", "negative_src", "kind_7", "kind_negative"])
def test_a_plan_row_that_does_not_fit_leaves_its_document_blank(case):
    ids, want = _valid()
    plan, kinds = want["plan"].copy(), want["kinds"].copy()
    i = int(np.flatnonzero((want["kinds"] != R.PLAIN) & (plan[:, 1] >= 8))[3])
    if case == "lo_above_hi":
        plan[i, 2], plan[i, 3] = plan[i, 3] + 1, plan[i, 3]
    elif case == "hi_above_n":
        plan[i, 3] = plan[i, 1] + 1
    elif case == "past_the_ids":
        plan[i, 0] = len(ids) - plan[i, 1] + 1
    elif case == "negative_src":
        plan[i, 0] = -1
    else:
        kinds[i] = 7 if case == "kind_7" else -1
    got = run_render(ids, plan, kinds, want["out_offsets"])
    assert got["err"][1] == _capi.E_ARG
    n_out = len(want["out_ids"])
    assert_guard(got, n_out)
    o0, o1 = want["out_offsets"][i], want["out_offsets"][i + 1]
    assert (got["out_ids"][o0:o1] == 0).all() and (got["labels"][o0:o1] == IGN).all()
    assert (got["parts"][o0:o1] == -1).all() and (got["source"][o0:o1] == -1).all()
    for k in PER_TOKEN:  # every other document is as ever
        assert np.array_equal(got[k][:o0], want[k][:o0]) and np.array_equal(got[k][o1:n_out], want[k][o1:])


@pytest.mark.parametrize("case", ["one_longer", "one_shorter", "first_is_not_0", "decreasing", "past_the_capacity"])
def test_out_offsets_that_are_not_the_scan_are_reported(case):
    ids, want = _valid(8)
    oo = want["out_offsets"].copy()
    if case == "one_longer":
        oo[40] += 1
    elif case == "one_shorter":
        oo[40] -= 1
    elif case == "first_is_not_0":
        oo[0] = 2
    elif case == "decreasing":
        oo[30:60] = oo[30:60][::-1].copy()
    else:
        oo[-1] += 5 * S
    got = run_render(ids, want["plan"], want["kinds"], oo)
    assert _capi.E_ARG in got["err"][1:] or got["err"][1] == _capi.E_CAPACITY
    assert got["err"][1] != 0
    assert_guard(got, got["cap"])


def test_capacity():
    ids, want = _valid(9)
    n_out = len(want["out_ids"])
    got = run_render(ids, want["plan"], want["kinds"], want["out_offsets"], out_cap=n_out - 1)
    assert got["err"][1] == _capi.E_CAPACITY
    for k in PER_TOKEN:
        assert np.array_equal(got[k][:n_out - 1], want[k][:n_out - 1])
    assert_guard(got, n_out - 1)
    got = run_render(ids, want["plan"], want["kinds"], want["out_offsets"], out_cap=n_out)
    assert got["err"][1] == 0
    got = run_render(ids, want["plan"], want["kinds"], want["out_offsets"], out_cap=0)
    assert got["err"][1] == _capi.E_CAPACITY
    assert_guard(got, 0)


def test_pieces_that_do_not_fit_are_reported():
    b = Forced(4)
    for k in range(50):
        b.doc(6, 2, 4, (R.PSM, R.SPM)[k % 2])
    for case in ("kind", "decreasing", "past"):
        offsets, kinds = list(b.offsets), list(b.kinds)
        if case == "kind":
            kinds[10] = 7
        elif case == "decreasing":
            offsets[3 * 10 + 1] = offsets[3 * 10] - 1
        else:
            offsets[-1] += 9
        got = run_pieces(b.ids, offsets, kinds)
        assert got["err"][0] == _capi.E_ARG
        assert_guard(got, got["cap"])


def test_no_documents():
    got = run_tokens([], [0], seed=1, fb=ONE, sb=ONE)
    assert got["err"] == [0, 0] and got["out_offsets"].tolist() == [0]
    assert_guard(got, 0)


# ---- the text cut ------------------------------------------------------------------------------------------------------------
def run_cut(data, offsets, *, seed, fb, sb, first=0, off=0, n_bytes=None):
    import torch
    n_docs = len(offsets) - 1
    d_bytes, d_offs = _dev(np.frombuffer(bytes(data), dtype=np.uint8).copy(), np.uint8, off), _dev(offsets, np.int64, off)
    pieces, kinds = _dev([SENT64] * (3 * n_docs + 1 + GUARD), np.int64, off), _dev([SENT32] * (n_docs + GUARD), np.int32, off)
    err = _dev([-7], np.int32)
    _capi.fim_cut_text_device(d_bytes.data_ptr(), d_offs.data_ptr(), n_docs, len(data) if n_bytes is None else n_bytes, seed, first,
                              fb, sb, pieces.data_ptr(), kinds.data_ptr(), err.data_ptr(), 0)
    try:
        torch.cuda.synchronize()
        pieces, kinds, err = pieces.cpu().numpy(), kinds.cpu().numpy(), err.cpu().numpy().tolist()
    except RuntimeError as ex:
        pytest.exit("device failure, nothing more is run: %s" % ex, returncode=3)
    assert (pieces[3 * n_docs + 1:] == SENT64).all() and (kinds[n_docs:] == SENT32).all()
    return pieces[:3 * n_docs + 1], kinds[:n_docs], err[0]


def pack(docs):
    docs = [d.encode() if isinstance(d, str) else bytes(d) for d in docs]
    return b"".join(docs), np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)


def test_text_cut_keeps_characters_whole():
    docs = ["plain ascii, nothing else", "", "éáűőúöüóí" * 2, "", "日本語のテキストです", "🙂🙃😀😎🤖", "a", "é", "🙂"] * 60
    data, offsets = pack(docs)
    lens = np.diff(offsets)
    for seed, off in ((1, 0), (2, 1)):
        _kind, lo, hi = R.decide(seed, np.arange(len(docs)), lens, ONE, ONE // 2)
        for width, text in ((2, "éáűőúöüóí" * 2), (3, "日本語のテキストです"), (4, "🙂🙃😀😎🤖")):
            mine = np.array([d == text for d in docs])
            assert {int(c) % width for c in np.concatenate([lo[mine], hi[mine]])} == set(range(width))   # every continuation byte is met
        want_p, want_k = R.cut_text(data, offsets, seed=seed, fim_below=ONE, spm_below=ONE // 2)
        pieces, kinds, err = run_cut(data, offsets, seed=seed, fb=ONE, sb=ONE // 2, off=off)
        assert err == 0 and np.array_equal(pieces, want_p) and np.array_equal(kinds, want_k)
        assert (np.diff(pieces) >= 0).all() and pieces[-1] == len(data)
        for i, d in enumerate(docs):
            parts = [data[pieces[3 * i + k]:pieces[3 * i + k + 1]].decode("utf-8") for k in range(3)]   # each piece decodes
            assert "".join(parts) == d and (kinds[i] == R.PLAIN) == (d == "")
    want_p, want_k = R.cut_text(data, offsets, seed=3, fim_below=ONE // 2, spm_below=ONE // 2, first_doc=2**33)
    pieces, kinds, err = run_cut(data, offsets, seed=3, fb=ONE // 2, sb=ONE // 2, first=2**33)
    assert err == 0 and np.array_equal(pieces, want_p) and np.array_equal(kinds, want_k) and set(kinds.tolist()) == {0, 1, 2}
    plain = kinds == R.PLAIN
    assert np.array_equal(pieces[1:-1:3][plain], offsets[1:][plain]) and np.array_equal(pieces[2::3][plain], offsets[1:][plain])
    pieces, kinds, err = run_cut(data, offsets, seed=3, fb=0, sb=0)
    assert err == 0 and (kinds == 0).all() and np.array_equal(pieces[0::3], offsets)


def test_text_cut_goes_at_most_three_steps_back():
    doc = b"a" + b"\x80" * 5 + b"b"
    data, offsets = pack([doc] * 400)
    _kind, lo, hi = R.decide(5, np.arange(400), len(doc), ONE, 0)
    assert (lo == 5).any() and (hi == 5).any() and (lo == 4).any()
    want_p, want_k = R.cut_text(data, offsets, seed=5, fim_below=ONE, spm_below=0)
    pieces, kinds, err = run_cut(data, offsets, seed=5, fb=ONE, sb=0)
    assert err == 0 and np.array_equal(pieces, want_p) and np.array_equal(kinds, want_k)
    i = int(np.flatnonzero(lo == 5)[0])
    assert pieces[3 * i + 1] - pieces[3 * i] == 2                                    # 5 -> 2, not to the 'a'


def test_text_cut_without_text_and_with_offsets_that_do_not_fit():
    pieces, kinds, err = run_cut(b"", [0, 0, 0, 0], seed=1, fb=ONE, sb=ONE)
    assert err == 0 and pieces.tolist() == [0] * 10 and kinds.tolist() == [0, 0, 0]
    pieces, kinds, err = run_cut(b"", [0], seed=1, fb=ONE, sb=ONE)
    assert err == 0 and pieces.tolist() == [0]
    data, offsets = pack(["some text here"] * 20)
    for case in ("decreasing", "past", "end", "start"):
        o, n_bytes = offsets.copy(), len(data)
        if case == "decreasing":
            o[7] = o[6] - 3
        elif case == "past":
            o[7:] += 10 * len(data)
        elif case == "end":
            n_bytes -= 1
        else:
            o[0] = 1
        pieces, kinds, err = run_cut(data, o, seed=1, fb=ONE, sb=ONE // 2, n_bytes=n_bytes)
        assert err == _capi.E_ARG
        if case in ("decreasing", "past"):
            assert kinds[7 if case == "past" else 6] == R.PLAIN


# ---- composition with the VG vocabulary (byte-level) -------------------------------------------------------------------------
TEXTS = ["def add(a, b):\n    return a + b\n", "", "x", "árvíztűrő tükörfúrógép: " * 3, "日本語のテキストも切れる。" * 2,
         "for i in range(10):\n    print(i)  # 🙂 emoji inside a comment\n", "class A:\n    pass\n" * 4, "é"] * 5


@pytest.fixture(scope="module")
def vg():
    import hutoken_amd
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, prefix=kw["prefix"], is_byte_encoder=kw["is_byte_encoder"], device=0)
    return hutoken_amd


def encode_all(H, texts):
    """batch_encode, with [] for an empty text"""
    some = iter(H.batch_encode([t for t in texts if t]))
    return [next(some) if t else [] for t in texts]


def padded(rows, L, pad):
    return np.array([list(r[:L]) + [pad] * (L - len(r[:L])) for r in rows], dtype=np.int64).reshape(len(rows), L)


def arrange(kind, pre, mid, suf, end, loss_bits):
    """the three encoded pieces of one document -> (ids, labels) by the rule"""
    def part(tokens, p):
        return [(t, t if (loss_bits >> p) & 1 else IGN) for t in tokens]

    def sentinel(t, is_end=False):
        return [(t, t if (loss_bits >> 4) & 1 or (is_end and loss_bits & R.LOSS_END) else IGN)]
    if kind == R.PLAIN:
        seq = part(pre + mid + suf, 0)
    else:
        tail = sentinel(END, True) if end is not None else []
        if kind == R.PSM:
            seq = sentinel(PRE) + part(pre, 1) + sentinel(SUF) + part(suf, 3) + sentinel(MID) + part(mid, 2) + tail
        else:
            seq = sentinel(PRE) + sentinel(SUF) + part(suf, 3) + sentinel(MID) + part(pre, 1) + part(mid, 2) + tail
    return [t for t, _l in seq], [l for _t, l in seq]


def test_batch_encode_fim_char_level_equals_the_host_composition(vg):
    import torch
    H = vg
    data, offsets = pack(TEXTS)
    sent = dict(prefix_id=PRE, suffix_id=SUF, middle_id=MID)
    for seed, end, loss_on, bits, dtype, max_length in ((1, END, "all", R.LOSS_ALL, torch.int32, None),
                                                        (2, None, "middle", R.LOSS_MIDDLE, torch.int64, 24),
                                                        (3, END, "middle", R.LOSS_MIDDLE, None, None)):
        pieces, kinds = R.cut_text(data, offsets, seed=seed, fim_below=int(0.7 * ONE), spm_below=ONE // 2, first_doc=5)
        texts = [data[pieces[k]:pieces[k + 1]].decode("utf-8") for k in range(3 * len(TEXTS))]
        enc = encode_all(H, texts)
        rows = [arrange(kinds[i], enc[3 * i], enc[3 * i + 1], enc[3 * i + 2], end, bits) for i in range(len(TEXTS))]
        L = max(len(r[0]) for r in rows) if max_length is None else max_length
        ids, mask, lengths, labels = H.batch_encode_fim(TEXTS, max_length, seed=seed, fim_rate=0.7, first_doc=5, end_id=end,
                                                        loss_on=loss_on, pad_id=-7, dtype=dtype, **sent)
        assert ids.shape == labels.shape == (len(TEXTS), L) and ids.dtype == labels.dtype == (dtype or torch.int32)
        assert np.array_equal(ids.cpu().numpy(), padded([r[0] for r in rows], L, -7))
        assert np.array_equal(labels.cpu().numpy(), padded([r[1] for r in rows], L, IGN))
        assert lengths.tolist() == [min(len(r[0]), L) for r in rows]
        assert set(kinds.tolist()) == {0, 1, 2}
    res = H.batch_encode_fim(TEXTS, seed=1, return_plan=True, **sent)
    assert len(res) == 5 and res[4].shape == (len(TEXTS), 8)
    # fim_rate 0: the plain batch
    ids, mask, lengths, labels = H.batch_encode_fim(TEXTS, seed=1, fim_rate=0.0, **sent)
    want = encode_all(H, TEXTS)
    assert np.array_equal(ids.cpu().numpy(), padded(want, ids.shape[1], 0)) and lengths.tolist() == [len(r) for r in want]


def test_the_source_gives_the_text_back(vg):
    import torch
    H = vg
    data, offsets = pack(TEXTS)
    d_bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    d_offs = torch.from_numpy(offsets).cuda()
    pieces, kinds = H.fim_cut_text_device(d_bytes, d_offs, seed=4, fim_rate=0.8, check=True)
    want_p, want_k = R.cut_text(data, offsets, seed=4, fim_below=int(0.8 * ONE), spm_below=ONE // 2)
    assert np.array_equal(pieces.cpu().numpy(), want_p) and np.array_equal(kinds.cpu().numpy(), want_k)
    ids, oo = H.encode_packed_device(d_bytes, pieces)
    out_ids, out_offsets, parts, source = H.fim_pieces_device(ids, oo, kinds, prefix_id=PRE, suffix_id=SUF, middle_id=MID, end_id=END,
                                                              return_parts=True, return_source=True, check=True)
    n_out = int(out_offsets[-1])
    ids_h, out_h, src_h, parts_h, oo_h = ids.cpu().numpy(), out_ids[:n_out].cpu().numpy(), source[:n_out].cpu().numpy(), \
        parts[:n_out].cpu().numpy(), out_offsets.cpu().numpy()
    assert ((src_h >= 0) == (parts_h != R.PART_SENTINEL)).all() and (out_h[src_h >= 0] == ids_h[src_h[src_h >= 0]]).all()
    for i, text in enumerate(TEXTS):
        src = src_h[oo_h[i]:oo_h[i + 1]]
        order = np.sort(src[src >= 0])            # prefix, middle, suffix: the pieces' order is the document's
        assert H.decode(ids_h[order].tolist()) == text if len(order) else text == ""
    # the spans of the pieces' tokens are carried over by the source
    spans = H.token_spans_device(d_bytes, pieces, ids, oo, unit="byte")
    carried = spans[source[:n_out][source[:n_out] >= 0]].cpu().numpy()
    piece_texts = [data[want_p[k]:want_p[k + 1]].decode("utf-8") for k in range(3 * len(TEXTS))]
    host_ids, host_spans = H.batch_encode_with_offsets([t for t in piece_texts if t], unit="byte")
    flat = np.array([list(s) for row in host_spans for s in row], dtype=np.int64).reshape(-1, 2)
    assert np.array_equal(carried, flat[src_h[src_h >= 0]])


def test_token_level_is_a_permutation_of_the_plain_ids(vg):
    H = vg
    plain = encode_all(H, TEXTS)
    ids, mask, lengths, labels = H.batch_encode_fim(TEXTS, seed=6, level="token", fim_rate=1.0, prefix_id=PRE, suffix_id=SUF,
                                                    middle_id=MID, end_id=END, loss_on="middle")
    ids, labels = ids.cpu().numpy(), labels.cpu().numpy()
    for i, row in enumerate(plain):
        got = ids[i][:int(lengths[i])].tolist()
        extra = [PRE, SUF, MID, END] if row else []
        assert sorted(got) == sorted(row + extra)
        on = labels[i][:int(lengths[i])] != IGN
        assert (labels[i][:int(lengths[i])][on] == ids[i][:int(lengths[i])][on]).all()


def test_fim_to_a_packed_training_batch(vg):
    import torch
    H = vg
    ids, oo = H._texts_to_device(TEXTS)
    n_ids = int(oo[-1])
    ids_h, oo_h = ids[:n_ids].cpu().numpy(), oo.cpu().numpy()
    want = R.fim_tokens(ids_h, oo_h, seed=8, fim_below=ONE // 2, spm_below=ONE // 2, pre=PRE, suf=SUF, mid=MID, end=END,
                        loss_parts=R.LOSS_MIDDLE, ignore_index=IGN)
    L = 32
    ref = packed_ref.Packer(L, pad_id=0, channels=[(np.int32, 1, IGN)])
    w_rows = packed_ref.cat([ref.add(want["out_ids"], want["out_offsets"], [want["labels"]]), ref.flush()])
    w_labels = packed_ref.labels_vec(w_rows["channels"][0], w_rows["segment_ids"], True, IGN)
    out_ids, out_oo, labels = H.fim_device(ids, oo, prefix_id=PRE, suffix_id=SUF, middle_id=MID, end_id=END, seed=8,
                                           loss_on="middle", return_labels=True, check=True)
    with H.SequencePacker(L, channels={"labels": ("int32", IGN)}) as packer:
        done = packer.add(out_ids, out_oo, check=True, channels={"labels": labels})
        rest = packer.flush()
    rows = {k: torch.cat([done[k], rest[k]]) for k in done}
    for k in ("input_ids", "position_ids", "segment_ids"):
        assert np.array_equal(rows[k].cpu().numpy(), w_rows[k]), k
    assert np.array_equal(rows["labels"].cpu().numpy(), w_rows["channels"][0])
    lab = H.packed_lm_labels(rows["labels"], rows["segment_ids"], shift=True)
    assert np.array_equal(lab.cpu().numpy(), w_labels) and (w_labels != IGN).any()
