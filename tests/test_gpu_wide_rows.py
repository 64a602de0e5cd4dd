"""The row passes, packed rows, the chat render and fill-in-the-middle on batches just past 2^31 and 2^32 ELEMENTS: flat
indices row * L + c and span bases, wavefront searches over offsets, and `source` and plan values that are negative as
int32 or wrap as uint32.  The builders, references and checkers are tests/wide_rows.py; tests/test_wide_rows_cpu.py
holds them to their claims without a GPU and shows that each of them fails on a wrapped index.

The row cases run on B // L + 64 int32 rows of L = 2048 columns, and of L = 2047, which takes the element path of every
VEC kernel and puts the boundary inside a row; a module-scoped fixture collates them once per parameter
(collate_padded(..., return_plan=True, check=True)).  Large inputs are drawn or repeated on the device and nothing of
an output's size is copied to the host.  Every case first asserts that the same call on a small batch (the first 1000
rows, the documents up to the first sync point, one block) equals the Python reference, so that a failure of the wide
batch is one of position.  What is compared:

    gather_rows (4 and 16 bytes)   the WHOLE rectangle against torch_gather; the band against features_ref.gather
    lm_labels                      the WHOLE rectangle against torch_lm_labels: "all" and ("a", "end"), shift on and off
    mask_tokens                    the band and the first 64 rows against targets_ref.mlm_ref; every element and the totals
                                   of the whole rectangle by mlm_invariants.  Whole-word mode takes a words array as long
                                   as the ids: the padded batch's ids are few (20 a row), so no words array past 2^31
                                   ids is needed for a rectangle past it
    corrupt_spans                  the band and the first 64 rows against span_ref.span_corrupt_ref; every row of the whole
                                   rectangle by span_invariants, which compares input_lengths and target_lengths whole with
                                   counts taken from the outputs
    packed_lm_labels               the WHOLE rectangle against torch_packed_labels, shift on and off
    SequencePacker with channels   one add() of more than B elements, then flush(): the rows between the sync points
                                   either side of the boundary and the tail with the flushed row against
                                   packed_ref.Packer; over everything the sum of input_ids and the count of real columns
    render_chat_device             EVERY copy of the block against chat_ref (out_ids, labels, turn_ids, source, out_offsets)
    fim_pieces_device              EVERY copy of the block against fim_ref (out_ids, labels, parts, source, out_offsets)
    the token-level plan + render  (the C entry points, which give the plan and the kinds; outputs inside guard bands)
                                   the documents around the place where the INPUT passes the boundary and around the one
                                   where the OUTPUT does against fim_ref.fim_tokens: out_ids, labels, parts, source, kinds,
                                   plan rows, out_offsets; over everything out_offsets, the total and the sum of out_ids

Memory: the rule and the line "WIDE | case | boundary | ran or skipped | bytes needed | bytes free | seconds" of
tests/test_gpu_wide_batches.py (wide_cases.Row; pytest -s, or -rs for the skips).
Measured on an MI355X, seconds per case (pytest's call time) at 2^31 with L = 2048 / 2^31 with L = 2047 / 2^32: the padded rows
(set-up) 2.0 / 0.3 / 0.3; gather_rows of 4 bytes 0.9 / 0.2 / 0.3, of 16 bytes 0.7 / 2.5 / 3.7; lm_labels 0.5 / 0.3 / 0.3, with
shift 0.3 / 0.3 / 0.4; mask_tokens 0.3 / 0.4 / 0.4, whole words 0.6 / 0.4 / 3.6; corrupt_spans 0.4 / 0.3 / 0.5;
packed_lm_labels 0.3 / 0.3 / 0.3; SequencePacker with channels 5.0 / 4.2 / skipped (it needs 249 458 211 120 bytes, 56 per
element of the stream: with 286 487 740 416 free the 1.25 x rule cannot hold at 2^32).  At 2^31 / 2^32: render_chat_device
0.6 / 4.3, fim_pieces_device 0.7 / 4.4, the token-level plan and render 0.5 / 4.6.  The file 46 s;
test_more_than_2_to_the_31_elements of tests/test_gpu_collate.py, the yardstick, 1.9 s in the same run.
Needs a real MI355X."""
import numpy as np
import pytest

import features_ref
import fim_ref
import packed_ref
import targets_ref as T
import wide_cases as W
import wide_rows as WR
from wide_cases import Row

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCRATCH = 3 * 2 ** 30  # what the comparisons themselves allocate
SMALL = 1000           # the rows of a case's first assertion
SEED = 2 ** 40 + 17
ROW_PARAMS = [pytest.param((W.B31, 2048), id="2^31-L2048"), pytest.param((W.B31, 2047), id="2^31-L2047"),
              pytest.param((W.B32, 2048), id="2^32-L2048")]
BOUNDARIES = [pytest.param(W.B31, id="2^31"), pytest.param(W.B32, id="2^32")]


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.cpu().numpy()


class Padded:
    """The padded batch of one parameter: ids, offs (device and host), rows, mask, lengths, plan"""

    def __init__(self, B, L):
        import torch
        import hutoken_amd
        self.B, self.L = B, L
        self.lens, self.offs, _tr, _em = WR.padded_docs(B, L)
        self.n, self.n_ids = len(self.lens), int(self.offs[-1])
        self.band = WR.band(B, L)
        self.ids = WR.draw_ids(self.n_ids, DEV)
        self.rows, self.mask, self.lengths, self.plan = hutoken_amd.collate_padded(
            self.ids, dev(self.offs), L, bos_id=WR.BOS, eos_id=WR.EOS, pad_id=WR.PAD, truncation="left", n_ids=self.n_ids,
            return_plan=True, check=True)
        torch.cuda.synchronize()
        assert self.rows.shape == (self.n, L) and self.rows.numel() >= B + 63 * L and self.rows.dtype == torch.int32
        self.elems = self.n * L
        # the collation itself is tests/test_gpu_collate.py's; here, its band against the plan the references are given
        a, b = self.band
        want = features_ref.padded_plan(self.offs[a:b + 1] - self.offs[a], L, bos_id=WR.BOS, eos_id=WR.EOS, truncation="left")
        want[:, 0] += a
        want[:, 2] += self.offs[a]
        assert np.array_equal(host(self.plan[a:b]), want), "the plan of the band"

    def places(self):
        """(first row, end) of the rows the Python references are run on: the first 64 and the band"""
        return ((0, 64), self.band)


@pytest.fixture(scope="module", params=ROW_PARAMS)
def padded(request):
    import gc
    import torch
    B, L = request.param
    n = WR.rows_shape(B, L) * L
    with Row("the padded rows, L = %d" % L, B, 5 * n + 64 * (n // L) + 2 ** 30):
        p = Padded(B, L)
    yield p
    p.__dict__.clear()
    del p
    gc.collect()
    torch.cuda.empty_cache()


# ---- gather_rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", [4, 16])
def test_gather_rows(padded, rec):
    import hutoken_amd
    p, L, B = padded, padded.L, padded.B
    with Row("gather_rows, %d-byte records, L = %d" % (rec, L), B, rec * p.elems + 20 * p.n_ids + SCRATCH):
        values = WR.gather_values(p.n_ids, DEV)[rec == 16]
        fill = WR.FILL4 if rec == 4 else WR.FILL16

        def reference(a, b):  # features_ref.gather on rows [a, b), given only their values
            plan = host(p.plan[a:b])
            lo, hi = int(p.offs[a]), int(p.offs[b])
            plan[:, 2] -= lo
            return features_ref.gather(plan, L, host(values[lo:hi]), fill=fill)
        small = hutoken_amd.gather_rows(p.plan[:SMALL], L, values, fill=fill, check=True)
        assert np.array_equal(host(small), reference(0, SMALL)), "the first %d rows alone differ from features_ref.gather" % SMALL
        del small
        out = hutoken_amd.gather_rows(p.plan, L, values, fill=fill, check=True)
        assert out.shape[:2] == (p.n, L) and out.numel() * out.element_size() == rec * p.elems
        WR.assert_rect(out, lambda a, b: WR.torch_gather(p.plan[a:b], L, values, fill), B, "gather_rows", slice_rows=8192)
        a, b = p.band
        WR.assert_band(out, reference(a, b), a, B, "gather_rows, the band")
        del out, values


# ---- lm_labels --------------------------------------------------------------------------------------------------------
LOSS = [("all", 15), (("a", "end"), T.LABELS_A | T.LABELS_END)]


@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shift"])
def test_lm_labels(padded, shift):
    import hutoken_amd
    p, L, B = padded, padded.L, padded.B
    with Row("lm_labels, shift %s, L = %d" % (shift, L), B, 4 * p.elems + SCRATCH):
        for loss_on, flags in LOSS:
            flags |= T.LABELS_SHIFT if shift else 0
            small = hutoken_amd.lm_labels(p.rows[:SMALL], p.mask[:SMALL], p.plan[:SMALL], loss_on=loss_on, shift=shift, check=True)
            want, wrong = T.labels_ref(host(p.rows[:SMALL]), host(p.mask[:SMALL]), host(p.plan[:SMALL]), flags, WR.IGN)
            assert not wrong and np.array_equal(host(small), want), "the first %d rows alone differ from labels_ref" % SMALL
            del small
            labels = hutoken_amd.lm_labels(p.rows, p.mask, p.plan, loss_on=loss_on, shift=shift, check=True)
            WR.assert_rect(labels, lambda a, b: WR.torch_lm_labels(p.rows[a:b], p.mask[a:b], p.plan[a:b], flags), B,
                           "lm_labels(%r, shift=%s)" % (loss_on, shift), slice_rows=32768)
            del labels


# ---- mask_tokens ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole_word", [False, True], ids=["tokens", "words"])
def test_mask_tokens(padded, whole_word):
    import torch
    import hutoken_amd
    p, L, B = padded, padded.L, padded.B
    with Row("mask_tokens, %s, L = %d" % ("words" if whole_word else "tokens", L), B, 8 * p.elems + 4 * p.n_ids + SCRATCH):
        words = None
        if whole_word:  # words of three tokens, every eleventh token protected
            i = torch.arange(p.n_ids, dtype=torch.int64, device=DEV)
            words = torch.where(i % 11 == 0, torch.full_like(i, -1), i // 3).to(torch.int32)
            del i
        kw = dict(mask_id=WR.MASK_ID, vocab_size=WR.VOCAB, seed=SEED, word_ids=words, check=True)
        out, labels = hutoken_amd.mask_tokens(p.rows[:SMALL], p.plan[:SMALL], **kw)
        want = WR.mlm_band(p.rows, p.plan, 0, SMALL, seed=SEED, words=words)
        assert np.array_equal(host(out), want[0]) and np.array_equal(host(labels), want[1]), \
            "the first %d rows alone differ from mlm_ref" % SMALL
        del out, labels
        out, labels = hutoken_amd.mask_tokens(p.rows, p.plan, **kw)
        for a, b in p.places():
            want = WR.mlm_band(p.rows, p.plan, a, b, seed=SEED, words=words)
            WR.assert_band(out, want[0], a, B, "mask_tokens, input_ids")
            WR.assert_band(labels, want[1], a, B, "mask_tokens, labels")
        counts = WR.mlm_invariants(p.rows, p.plan, out, labels, B, words=words, word_len=3 if whole_word else 1, slice_rows=32768)
        print("mask_tokens: %d eligible, %d selected, %d mask ids, %d random ids" % counts)
        del out, labels, words


# ---- corrupt_spans ----------------------------------------------------------------------------------------------------
def test_corrupt_spans(padded):
    import hutoken_amd
    p, L, B = padded, padded.L, padded.B
    with Row("corrupt_spans, L = %d" % L, B, 13 * p.elems + SCRATCH):
        kw = dict(sentinel_first=WR.SENT_FIRST, n_sentinels=WR.N_SENT, seed=SEED, target_eos_id=WR.EOS, decoder_start_id=WR.DEC_START,
                  pad_id=WR.PAD, check=True)
        names = ("input_ids", "attention_mask", "labels", "input_lengths", "target_lengths", "decoder_input_ids")
        res = hutoken_amd.corrupt_spans(p.rows[:SMALL], p.mask[:SMALL], p.plan[:SMALL], **kw)
        for name, got, want in zip(names, res, WR.span_band(p.rows, p.mask, p.plan, 0, SMALL, seed=SEED)):
            assert np.array_equal(host(got), want), "%s of the first %d rows alone differs from span_corrupt_ref" % (name, SMALL)
        del res
        res = hutoken_amd.corrupt_spans(p.rows, p.mask, p.plan, **kw)
        assert res[2].shape == (p.n, L)
        for a, b in p.places():
            for name, got, want in zip(names, res, WR.span_band(p.rows, p.mask, p.plan, a, b, seed=SEED)):
                WR.assert_band(got, want, a, B, "corrupt_spans, " + name)
        WR.span_invariants(p.mask, *res, B, slice_rows=32768)
        del res


# ---- packed_lm_labels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", ROW_PARAMS)
def test_packed_lm_labels(param):
    import torch
    import hutoken_amd
    B, L = param
    n = WR.rows_shape(B, L)
    with Row("packed_lm_labels, L = %d" % L, B, 12 * n * L + SCRATCH):
        values = WR.draw_ids(n * L, DEV, lo=-5, hi=50000).view(n, L)
        seg = torch.empty((n, L), dtype=torch.int32, device=DEV)
        for a in range(0, n, 32768):  # (the segment rows by a formula of row and column, on the device)
            seg[a:a + 32768] = WR.segment_rows(a, min(n, a + 32768), L, DEV)
        for shift in (False, True):
            small = hutoken_amd.packed_lm_labels(values[:SMALL], seg[:SMALL], shift=shift)
            assert np.array_equal(host(small), packed_ref.labels_vec(host(values[:SMALL]), host(seg[:SMALL]), shift, WR.IGN)), \
                "the first %d rows alone differ from packed_ref" % SMALL
            del small
            labels = hutoken_amd.packed_lm_labels(values, seg, shift=shift)
            WR.assert_rect(labels, lambda a, b: WR.torch_packed_labels(values[a:b], seg[a:b], shift), B,
                           "packed_lm_labels(shift=%s)" % shift, slice_rows=32768)
            del labels
        del values, seg


# ---- SequencePacker with channels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("param", ROW_PARAMS)
def test_sequence_packer_with_channels(param):
    import torch
    import hutoken_amd
    B, L = param
    s = WR.packed_stream(B, L)
    with Row("SequencePacker with channels, seq_len = %d" % L, B, 24 * s.n_ids + 8 * s.n_docs + 32 * s.total + SCRATCH):
        ids = WR.draw_ids(s.n_ids, DEV, lo=1000, hi=50000)
        offs = dev(s.offs)
        c4 = torch.empty(s.n_ids, dtype=torch.int32, device=DEV)
        c16 = torch.empty((s.n_ids, 2), dtype=torch.int64, device=DEV)
        for a in range(0, s.n_ids, 2 ** 26):
            c4[a:a + 2 ** 26], c16[a:a + 2 ** 26] = WR.channel_values(a, min(s.n_ids, a + 2 ** 26), DEV)
        chans = {"c4": c4, "c16": c16}

        def ids_of(d0, d1):
            return host(ids[int(s.offs[d0]):int(s.offs[d1])])
        # the documents up to the first sync point alone
        d1 = s.sync[1]
        with hutoken_amd.SequencePacker(L, eos_id=WR.EOS, pad_id=WR.PAD, channels=WR.PACK_CHANNELS) as packer:
            rows = packer.add(ids, offs[:d1 + 1], n_ids=int(s.offs[d1]), check=True, channels=chans)
            assert packer.pending == 0 and rows["input_ids"].shape == (s.start(d1) // L, L)
            WR.assert_packed_band(rows, WR.packed_rows_ref(s, ids_of(0, d1), 0, d1), 0, B, "the first documents alone")
            del rows
        # everything in one add
        with hutoken_amd.SequencePacker(L, eos_id=WR.EOS, pad_id=WR.PAD, channels=WR.PACK_CHANNELS) as packer:
            rows = packer.add(ids, offs, n_ids=s.n_ids, check=True, channels=chans)
            assert packer.pending == s.total % L > 0
            tail = packer.flush()
            torch.cuda.synchronize()
            n_rows = s.total // L
            assert rows["input_ids"].shape == (n_rows, L) and n_rows * L > B and tail["input_ids"].shape == (1, L)
            assert rows["c16"].shape == (n_rows, L, 2) and rows["c4"].dtype == torch.int32 and rows["c16"].dtype == torch.int64
            d0, d1, row0, row1 = s.band(B)
            assert row0 * L <= B < row1 * L
            WR.assert_packed_band(rows, WR.packed_rows_ref(s, ids_of(d0, d1), d0, d1), row0, B, "the rows between the sync points")
            dt, rowt = s.tail()
            want = WR.packed_rows_ref(s, ids_of(dt, s.n_docs), dt, s.n_docs, flush=True)
            assert len(want["input_ids"]) == n_rows - rowt + 1
            last = {k: v[-1:] for k, v in want.items() if k != "channels"}
            last["channels"] = [c[-1:] for c in want["channels"]]
            want = {k: v[:-1] for k, v in want.items() if k != "channels"} | {"channels": [c[:-1] for c in want["channels"]]}
            WR.assert_packed_band(rows, want, rowt, B, "the rows behind the last sync point")
            WR.assert_packed_band(tail, last, 0, B, "the flushed row")
            sum_ids = sum(int(ids[a:a + 2 ** 28].sum(dtype=torch.int64)) for a in range(0, s.n_ids, 2 ** 28))
            WR.packed_totals([rows, tail], sum_ids, s.n_docs, s.n_ids)
            del rows, tail
        del ids, offs, c4, c16, chans


# ---- the chat render ----------------------------------------------------------------------------------------------------
_blocks = {}


def block(kind):
    if kind not in _blocks:
        _blocks[kind] = (WR.chat_block if kind == "chat" else WR.fim_block)(W.B31, W.B32)
    return _blocks[kind]


def copies_of(b, boundary):
    """R: input and output both pass the boundary; the place p of the laid-out structures is where the OUTPUT does"""
    R = W.copies_cross(min(b.n_ids, b.n_out), boundary)
    assert R * b.n_ids >= boundary + 2 ** 26 and R * b.n_out >= boundary + 2 ** 26
    return R


def assert_block_alone(got, want, keys, what):
    n_out = len(want["out_ids"])
    assert np.array_equal(host(got["out_offsets"]), want["out_offsets"]), "%s: out_offsets of the block alone" % what
    for k in keys:
        assert np.array_equal(host(got[k][:n_out]), want[k]), "%s: %s of the block alone differs from the reference" % (what, k)


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_render_chat(boundary):
    import hutoken_amd
    b = block("chat")
    R = copies_of(b, boundary)
    tpl = WR.CHAT_TPL
    roles = {"r%d" % i: (tpl.prefix[i], tpl.suffix[i], tpl.suffix_loss[i]) for i in range(3)}
    template = hutoken_amd.ChatTemplate(roles, bos_id=tpl.bos, eos_id=tpl.eos)
    cap = tpl.bound(R * b.n_conv, R * b.n_turns, R * b.n_ids)
    keys = ("out_ids", "labels", "turn_ids", "source")
    try:
        with Row("render_chat_device with turn ids and source", boundary, 4 * R * b.n_ids + 28 * R * b.n_turns + 20 * cap + SCRATCH):
            def render(ids, offs, conv, role_ids, n_ids):
                res = hutoken_amd.render_chat_device(ids, offs, conv, role_ids, template, loss_roles=("r0", "r1"), n_ids=n_ids,
                                                     return_turn_ids=True, return_source=True, check=True)
                return dict(zip(("out_ids", "out_offsets", "labels", "turn_ids", "source"), res))
            got = render(dev(b.ids), dev(b.offsets), dev(b.conv), dev(b.roles), b.n_ids)
            assert_block_alone(got, b.ref, keys, "chat")
            del got
            got = render(dev(b.ids).repeat(R), WR.copies(b.offsets, b.n_ids, R, DEV), WR.copies(b.conv, b.n_turns, R, DEV),
                         dev(b.roles).repeat(R), R * b.n_ids)
            WR.assert_copy_offsets(got["out_offsets"], b.ref["out_offsets"], R, boundary, "chat, out_offsets")
            for k in keys:
                WR.assert_copies(got[k][:R * b.n_out], b.ref[k], R, b.n_ids if k == "source" else 0, boundary, "chat, " + k)
            del got
    finally:
        template.close()


# ---- fill-in-the-middle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_fim_pieces(boundary):
    import hutoken_amd
    from hutoken_amd import _capi
    b = block("fim")
    R = copies_of(b, boundary)
    cap = _capi.fim_ids_bound(R * b.n_docs, R * b.n_ids, True)
    keys = ("out_ids", "labels", "parts", "source")
    with Row("fim_pieces_device", boundary, 4 * R * b.n_ids + 70 * R * b.n_docs + 20 * cap + SCRATCH):
        def render(ids, offs, kinds, n_ids):
            res = hutoken_amd.fim_pieces_device(ids, offs, kinds, prefix_id=WR.PRE, suffix_id=WR.SUF, middle_id=WR.MID, end_id=WR.END,
                                                loss_on="middle", n_ids=n_ids, return_labels=True, return_parts=True,
                                                return_source=True, check=True)
            return dict(zip(("out_ids", "out_offsets", "labels", "parts", "source"), res))
        got = render(dev(b.ids), dev(b.offsets), dev(b.kinds), b.n_ids)
        assert_block_alone(got, b.ref, keys, "fim pieces")
        del got
        got = render(dev(b.ids).repeat(R), WR.copies(b.offsets, b.n_ids, R, DEV), dev(b.kinds).repeat(R), R * b.n_ids)
        WR.assert_copy_offsets(got["out_offsets"], b.ref["out_offsets"], R, boundary, "fim pieces, out_offsets")
        for k in keys:
            WR.assert_copies(got[k][:R * b.n_out], b.ref[k], R, b.n_ids if k == "source" else 0, boundary, "fim pieces, " + k)
        del got


def fim_tokens_raw(ids, offs, n_docs, n_ids):
    """hutk_fim_plan_tokens_device and hutk_fim_render_device, every output inside guard bands -> (dict, whether the bands
    are as they were)"""
    import torch
    from hutoken_amd import _capi
    cap = _capi.fim_ids_bound(n_docs, n_ids, True)
    sizes = {"out_offsets": (n_docs + 1, torch.int64), "plan": (4 * n_docs, torch.int64), "kinds": (n_docs, torch.int32),
             "out_ids": (cap, torch.int32), "labels": (cap, torch.int32), "parts": (cap, torch.int32), "source": (cap, torch.int64)}
    bufs = {k: WR.guarded(n, dt, DEV) for k, (n, dt) in sizes.items()}
    g = {k: v for k, (v, _store) in bufs.items()}
    err = torch.zeros(2, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _capi.fim_plan_tokens_device(offs.data_ptr(), n_docs, n_ids, WR.FIM_SEED, 0, WR.FIM_FB, WR.FIM_SB, True, g["out_offsets"].data_ptr(),
                                 g["plan"].data_ptr(), g["kinds"].data_ptr(), err[0:].data_ptr(), stream)
    _capi.fim_render_device(ids.data_ptr(), g["plan"].data_ptr(), g["kinds"].data_ptr(), g["out_offsets"].data_ptr(), n_docs, n_ids,
                            WR.PRE, WR.SUF, WR.MID, WR.END, fim_ref.LOSS_MIDDLE, WR.IGN, cap, g["out_ids"].data_ptr(),
                            g["labels"].data_ptr(), g["parts"].data_ptr(), g["source"].data_ptr(), err[1:].data_ptr(), stream)
    torch.cuda.synchronize()
    assert err.tolist() == [0, 0], "the device-side error words: %s" % err.tolist()
    g["plan"] = g["plan"].view(n_docs, 4)
    return g, all(WR.untouched(store, sizes[k][0]) for k, (_v, store) in bufs.items())


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_fim_tokens(boundary):
    B = boundary
    lens, offs = WR.fim_docs(B, extra=2 ** 26)
    n_docs, n_ids = len(lens), int(offs[-1])
    with Row("fim at token level: plan and render", B, 24 * (n_ids + 4 * n_docs) + 60 * n_docs + SCRATCH):
        ids = WR.draw_ids(n_ids, DEV, lo=1000, hi=50000)
        offs_t = dev(offs)
        # the first 2000 documents alone
        d1 = 2000
        got, clean = fim_tokens_raw(ids, offs_t[:d1 + 1], d1, int(offs[d1]))
        assert clean, "written outside the outputs"
        WR.assert_fim_band(got, WR.fim_band(host(ids[:int(offs[d1])]), offs, 0, d1), 0, d1, B)
        del got
        got, clean = fim_tokens_raw(ids, offs_t, n_docs, n_ids)
        assert clean, "written outside the outputs"
        n_moved = WR.fim_totals(got, offs_t, ids, n_ids)
        assert int(got["out_offsets"][-1]) >= B + 2 ** 26 and n_moved > n_docs // 3
        d_in = int(np.searchsorted(offs, B, side="right")) - 1                                        # the INPUT passes B inside it
        d_out = int((got["out_offsets"] <= B).sum()) - 1                                                # the OUTPUT does
        assert 64 < d_out < d_in < n_docs - 64
        for d in (d_out, d_in):
            d0, d1 = d - 64, d + 64
            want = WR.fim_band(host(ids[int(offs[d0]):int(offs[d1])]), offs, d0, d1)
            if d == d_in:
                assert want["plan"][:, 0].max() >= B and want["source"].max() >= B
            WR.assert_fim_band(got, want, d0, d1, B)
        del got, ids, offs_t
