"""The chat render on the GPU (hutk_chat_offsets_device, hutk_chat_render_device, render_chat_device, batch_encode_chat)
against chat_ref, element by element in all five outputs, on the smallest shapes at which the kernels can go wrong: the
edges of a workgroup's span, a turn longer than several spans, thousands of empty turns and sequences at one place, the
blocks of the scan, the template's limits, views off the 16-byte boundary, inputs the range checks must reject, and the
composition with encode, collation, packing and the token spans."""
import random

import numpy as np
import pytest

import chat_ref as R
from hutoken_amd import _capi

pytestmark = pytest.mark.gpu

IGN = -100
GUARD = 64
SENT32, SENT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
NO = _capi.NO_TOKEN

_handles = {}


def handle(tpl):
    h = _handles.get(id(tpl))
    if h is None:
        h = _handles[id(tpl)] = (_capi.ChatTemplate(list(zip(tpl.prefix, tpl.suffix)), tpl.suffix_loss,
                                                    NO if tpl.bos is None else tpl.bos, NO if tpl.eos is None else tpl.eos, 0), tpl)
    return h[0]


def _dev(values, dtype, off):
    """values on the GPU as a view `off` elements behind a 16-byte boundary"""
    import torch
    arr = np.asarray(values, dtype=dtype)
    base = torch.zeros(arr.size + off + 4, dtype=getattr(torch, np.dtype(dtype).name), device="cuda:0")
    view = base[off:off + arr.size]
    view.copy_(torch.from_numpy(arr))
    assert arr.size == 0 or view.data_ptr() % 16 == (off * arr.itemsize) % 16
    return view


def run(tpl, ids, offsets, roles, conv, gen=-1, loss=0, out_cap=None, off=0, n_ids=None, with_extra=True):
    """The two device calls on fresh, sentinel-filled outputs with a guard behind out_cap.  off = 1: every buffer is a view
    one element off the 16-byte boundary (4 bytes for the id-typed ones, 8 for the offsets and the source).
    -> dict of numpy arrays (the per-token ones whole: out_cap + GUARD elements) and the two error words."""
    import torch
    h = handle(tpl)
    n_turns, n_conv = len(offsets) - 1, len(conv) - 1
    n_ids = len(ids) if n_ids is None else n_ids
    cap = h.ids_bound(n_conv, n_turns, n_ids, gen) if out_cap is None else out_cap
    d_ids, d_offs = _dev(ids, np.int32, off), _dev(offsets, np.int64, off)
    d_roles, d_conv = _dev(roles, np.int32, off), _dev(conv, np.int64, off)
    T, oo = _dev([SENT64] * (n_turns + 1), np.int64, off), _dev([SENT64] * (n_conv + 1), np.int64, off)
    outs = {"out_ids": _dev([SENT32] * (cap + GUARD), np.int32, off), "labels": _dev([SENT32] * (cap + GUARD), np.int32, off)}
    if with_extra:
        outs["turn_ids"] = _dev([SENT32] * (cap + GUARD), np.int32, off)
        outs["source"] = _dev([SENT64] * (cap + GUARD), np.int64, off)
    err = _dev([-7, -7], np.int32, off)
    try:
        h.offsets_device(d_offs.data_ptr(), d_roles.data_ptr(), d_conv.data_ptr(), n_conv, n_turns, n_ids, gen, T.data_ptr(),
                         oo.data_ptr(), err[0:].data_ptr(), 0)
        h.render_device(d_ids.data_ptr(), d_offs.data_ptr(), d_roles.data_ptr(), d_conv.data_ptr(), T.data_ptr(), oo.data_ptr(),
                        n_conv, n_turns, n_ids, gen, loss, IGN, cap, outs["out_ids"].data_ptr(), outs["labels"].data_ptr(),
                        outs["turn_ids"].data_ptr() if with_extra else 0, outs["source"].data_ptr() if with_extra else 0,
                        err[1:].data_ptr(), 0)
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in outs.items()}
    except RuntimeError as ex:
        pytest.exit("device failure, nothing more is run: %s" % ex, returncode=3)
    res.update(turn_offsets=T.cpu().numpy(), out_offsets=oo.cpu().numpy(), err=err.cpu().numpy().tolist(), cap=cap)
    return res


PER_TOKEN = ("out_ids", "labels", "turn_ids", "source")


def assert_guard(got, n_written):
    """nothing is written at or behind `n_written` (the sequences' end, or the capacity)"""
    for k in PER_TOKEN:
        if k in got:
            tail = got[k][n_written:]
            assert (tail == (SENT64 if k == "source" else SENT32)).all(), "%s was written behind element %d" % (k, n_written)


def check(tpl, ids, offsets, roles, conv, gen=-1, loss=0, want_err=0, **kw):
    """all outputs equal chat_ref's, nothing written behind them -> (got, want)"""
    want = R.render(tpl, ids, offsets, roles, conv, gen_role=gen, loss_roles=loss, ignore_index=IGN)
    got = run(tpl, ids, offsets, roles, conv, gen=gen, loss=loss, **kw)
    assert max(got["err"]) == want_err == want["err"], got["err"]
    assert np.array_equal(got["turn_offsets"], want["turn_offsets"])
    assert np.array_equal(got["out_offsets"], want["out_offsets"])
    n_out = len(want["out_ids"])
    assert n_out <= got["cap"]
    for k in PER_TOKEN:
        if k in got:
            bad = np.nonzero(got[k][:n_out] != want[k])[0]
            assert bad.size == 0, "%s differs at %d of %d: got %d, want %d" % (k, bad[0], n_out, got[k][bad[0]], want[k][bad[0]])
    assert_guard(got, n_out)
    return got, want


class Batch:
    """conversations put together turn by turn"""

    def __init__(self, seed=0):
        self.rng = random.Random(seed)
        self.ids, self.offsets, self.roles, self.conv = [], [0], [], [0]

    def turn(self, role, n):
        self.ids += [self.rng.randrange(1000, 50000) for _ in range(n)]
        self.offsets.append(len(self.ids))
        self.roles.append(role)
        return self

    def end(self):
        self.conv.append(len(self.roles))
        return self

    def args(self):
        return self.ids, self.offsets, self.roles, self.conv


# role 0: prefix of 3, suffix of 2; role 1: prefix of 1, suffix of 2 with loss on the first; role 2: nothing at all
PARTS = ([[11, 12, 13], [21], []], [[14, 15], [22, 23], []])
TPL_BE = R.Template(*PARTS, suffix_loss=[2, 1, 0], bos=1, eos=2)
TPL_B = R.Template(*PARTS, suffix_loss=[2, 1, 0], bos=1)
TPL_0 = R.Template(*PARTS, suffix_loss=[2, 1, 0])
S = None


@pytest.fixture(scope="module", autouse=True)
def span():
    global S
    S = _capi.chat_span()
    assert S >= 64
    yield S
    for h, _tpl in _handles.values():
        h.close()
    _handles.clear()


# ---- span edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_conversations_that_end_at_a_span_edge(lead):
    """Rendered lengths S-1, S, S+1 and 2S, behind 0 to 3 one-token conversations ([bos] alone) that walk them over the
    boundary; and the same with an eos, behind conversations of two tokens."""
    for tpl, fixed in ((TPL_B, 1), (TPL_BE, 2)):
        for first in (S - 1, S, S + 1, 2 * S):
            b = Batch(lead)
            for _ in range(lead):
                b.end()
            for L in (first, S - 1, S, S + 1, 2 * S):
                b.turn(1, L - fixed - 3).end()  # role 1 adds 3
            got, want = check(tpl, *b.args(), loss=0b010)
            assert want["out_offsets"][lead + 1] - want["out_offsets"][lead] == first


def test_every_part_on_both_sides_of_a_span_edge():
    """bos, the prefix's start, the content's start, the suffix's start and eos of one turn, each on the last position
    of a span and on the first of the next."""
    c = 5
    for at in (0, 1, 4, 4 + c, 4 + c + 2):  # bos, prefix, content, suffix, eos inside [bos] 3 c 2 [eos]
        for pos in (S - 1, S, 2 * S - 1, 2 * S):
            lead = pos - at
            b = Batch(at).turn(1, lead - 2 - 3).end().turn(0, c).end().turn(1, 3).end()
            got, want = check(TPL_BE, *b.args(), loss=0b011)
            assert want["out_offsets"][1] == lead
            assert want["out_ids"][pos] == {0: 1, 1: 11, 4: b.ids[lead - 5], 4 + c: 14, 4 + c + 2: 2}[at]


def test_one_long_turn():
    """One content of 3S + 5 ids: the middle workgroups lie wholly inside one turn that began two spans back."""
    for tpl in (TPL_BE, TPL_0):
        b = Batch(1).turn(0, 7).turn(1, 3).end().turn(0, 2).turn(1, 3 * S + 5).turn(0, 1).end().turn(1, 4).end()
        check(tpl, *b.args(), loss=0b010)
    b = Batch(2).turn(2, 3 * S + 5).end()  # nothing but the content
    got, want = check(TPL_0, *b.args(), loss=0b100)
    assert np.array_equal(want["out_ids"], np.array(b.ids, dtype=np.int32))


# ---- zero-length turns and sequences --------------------------------------------------------------------------------------
def test_thousands_of_empty_turns_at_one_place():
    """5000 consecutive turns of rendered length 0 in front of a real one: inside one conversation, and across
    conversations (without bos and eos the sequences are empty too; with them they are two tokens each)."""
    for tpl in (TPL_0, TPL_BE):
        b = Batch(3).turn(0, 4)
        for _ in range(5000):
            b.turn(2, 0)
        b.turn(1, 6).end().turn(0, 2).end()
        check(tpl, *b.args(), loss=0b010)
        b = Batch(4).turn(0, 4).end()
        for _ in range(5000):
            b.turn(2, 0).end()
        b.turn(1, 6).end()
        got, want = check(tpl, *b.args(), loss=0b010)
        assert want["out_offsets"][-1] == 9 + 9 + 5002 * tpl.fixed()


def test_empty_conversations_with_equal_offsets():
    """fixed == 0: 3000 conversations without a token between two real ones; their out_offsets are equal and the searches
    must pick the real one.  Also where the place is a span's first position."""
    for n_first in (9, S - 5):  # the first conversation has n_first + 5 tokens
        b = Batch(5).turn(0, n_first).end()
        for k in range(3000):
            if k % 3 == 0:
                b.turn(2, 0)
            b.end()
        b.turn(1, 2 * S).end()
        got, want = check(TPL_0, *b.args(), loss=0b010)
        assert (want["out_offsets"][1:3002] == n_first + 5).all()


def test_more_than_a_thousand_sequences_in_one_span():
    """With bos and eos every empty conversation is two tokens: S/2 + 40 of them put over a thousand sequences in one
    span, a boundary between two of them, and one across it."""
    for lead in (0, 1):
        b = Batch(6)
        if lead:
            b.turn(2, 1).end()  # three tokens: the pairs behind it straddle the span's edge
        for k in range(S // 2 + 40):
            b.end()
        b.turn(0, 3).end()
        got, want = check(TPL_BE, *b.args(), loss=0b001)
    b = Batch(7)
    for k in range(S + 40):  # one-token sequences: a span full of starts
        b.end()
    check(TPL_B, *b.args())


# ---- the scan over the turns ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_turns", [255, 256, 257, 1000])
@pytest.mark.parametrize("one_conversation", [False, True])
def test_scan_edges(n_turns, one_conversation):
    b = Batch(n_turns)
    for _ in range(n_turns):
        b.turn(b.rng.randrange(3), b.rng.choice((0, 0, 1, 2, 5, 17)))
        if not one_conversation:
            b.end()
    if one_conversation:
        b.end()
    check(TPL_BE, *b.args(), loss=0b011)
    check(TPL_0, *b.args(), gen=1, loss=0b110)


# ---- the template's limits ------------------------------------------------------------------------------------------------
def test_template_limits():
    """16 roles; role 0 with a prefix and a suffix of 32 ids; suffix_loss of 0, 1 and all; loss_roles none, all and bit 15
    alone; a generation prompt for a role with an empty prefix and for one with 32 ids."""
    rng = random.Random(8)
    prefix = [[100 + k for k in range(32)]] + [[200 + 40 * r + k for k in range(rng.randrange(0, 6))] for r in range(1, 16)]
    suffix = [[150 + k for k in range(32)]] + [[900 + 40 * r + k for k in range(rng.randrange(1, 6))] for r in range(1, 16)]
    prefix[3] = []
    suffix_loss = [32, 0, 1] + [len(s) for s in suffix[3:]]
    suffix_loss[15] = 1
    for bos in (None, 1):
        tpl = R.Template(prefix, suffix, suffix_loss=suffix_loss, bos=bos)
        b = Batch(9)
        for c in range(40):
            for _ in range(rng.randrange(0, 7)):
                b.turn(rng.choice((0, 0, 1, 2, 3, 15, rng.randrange(16))), rng.choice((0, 1, 3, 40)))
            b.end()
        for loss in (0, 0xFFFF, 1 << 15):
            for gen in (-1, 3, 0):
                got, want = check(tpl, *b.args(), gen=gen, loss=loss)
                if loss == 0:
                    assert (want["labels"] == IGN).all()
    tpl = R.Template(prefix, suffix, suffix_loss=suffix_loss, bos=1, eos=2)
    check(tpl, *b.args(), loss=0xFFFF)
    b = Batch(10).turn(0, S - 70).turn(0, 0).turn(0, S).end()  # the longest parts over span edges
    check(tpl, *b.args(), loss=1)


def test_random_structures():
    rng = random.Random(11)
    for trial in range(12):
        n_roles = rng.randrange(1, 6)
        prefix = [[rng.randrange(1, 99) for _ in range(rng.randrange(0, 5))] for _ in range(n_roles)]
        suffix = [[rng.randrange(1, 99) for _ in range(rng.randrange(0, 4))] for _ in range(n_roles)]
        gen = rng.choice((-1, rng.randrange(n_roles)))
        tpl = R.Template(prefix, suffix, suffix_loss=[rng.randrange(len(s) + 1) for s in suffix], bos=rng.choice((None, 1)),
                         eos=rng.choice((None, 2)) if gen < 0 else None)
        b = Batch(trial)
        for _ in range(rng.randrange(1, 400)):
            for _ in range(rng.randrange(0, 9)):
                b.turn(rng.randrange(n_roles), rng.choice((0, 1, 2, 9, 60, 300)))
            b.end()
        check(tpl, *b.args(), gen=gen, loss=rng.randrange(1 << n_roles), with_extra=trial % 3 != 0)


# ---- views ------------------------------------------------------------------------------------------------------------------
def test_views_off_the_16_byte_boundary():
    """Every id-typed buffer one element (4 bytes) off the boundary, the offsets and the source 8 bytes off: the results of
    the aligned run."""
    b = Batch(12)
    for c in range(60):
        for _ in range(b.rng.randrange(0, 6)):
            b.turn(b.rng.randrange(3), b.rng.choice((0, 1, 7, 90, 700)))
        b.end()
    for tpl, gen in ((TPL_BE, -1), (TPL_0, 0)):
        a, want = check(tpl, *b.args(), gen=gen, loss=0b011)
        v, _ = check(tpl, *b.args(), gen=gen, loss=0b011, off=1)
        for k in PER_TOKEN + ("turn_offsets", "out_offsets"):
            assert np.array_equal(a[k], v[k]), k


# ---- inputs the range checks must reject ---------------------------------------------------------------------------------
def small_batch(seed=13):
    b = Batch(seed)
    b.turn(0, 5).turn(1, 7).end()
    b.turn(0, 3).turn(1, 4).turn(0, 6).end()
    b.turn(0, 2).turn(1, S + 9).end()
    b.turn(1, 8).end()
    return b


@pytest.mark.parametrize("role", [-1, 99])
def test_a_role_outside_the_template_leaves_its_turn_out(role):
    b = small_batch()
    b.roles[3] = role
    got, want = check(TPL_BE, *b.args(), loss=0b010, want_err=_capi.E_ARG)
    assert want["turn_offsets"][4] == want["turn_offsets"][3]
    b.roles[6] = role  # the long one too
    check(TPL_BE, *b.args(), loss=0b010, want_err=_capi.E_ARG)


def test_a_negative_turn_length_leaves_its_turn_out():
    b = small_batch()
    b.offsets[3], b.offsets[4] = b.offsets[4], b.offsets[3]  # turn 3 of conversation 1 runs backwards
    assert b.offsets[4] < b.offsets[3]
    check(TPL_BE, *b.args(), loss=0b010, want_err=_capi.E_ARG)


def test_a_turn_that_points_past_the_ids():
    """A length that can be (at most n_ids) at a place that cannot: the turn is rendered, what lies past n_ids is reported
    and undefined, and the conversations around it are exact."""
    b = small_batch()
    n_ids = len(b.ids)
    b.offsets[4] = n_ids + 3  # turn 3 reaches three ids past the end; turn 4 then has a negative length and is left out
    assert 0 <= b.offsets[4] - b.offsets[3] <= n_ids
    want = R.render(TPL_BE, *b.args(), loss_roles=0b010)
    # (turns that overlap render more ids than there are: the bound of hutk_chat_ids_bound does not cover them)
    got = run(TPL_BE, *b.args(), loss=0b010, out_cap=len(want["out_ids"]) + 5)
    assert got["err"] == [_capi.E_ARG, _capi.E_ARG] and want["err"] == _capi.E_ARG
    assert np.array_equal(got["turn_offsets"], want["turn_offsets"]) and np.array_equal(got["out_offsets"], want["out_offsets"])
    oo = want["out_offsets"]
    for i in (0, 2, 3):
        for k in PER_TOKEN:
            assert np.array_equal(got[k][oo[i]:oo[i + 1]], want[k][oo[i]:oo[i + 1]]), (k, i)
    inside = slice(oo[1], oo[2])  # the ids that exist are rendered in the damaged conversation too
    ok = want["source"][inside] >= 0
    assert np.array_equal(got["out_ids"][inside][ok], want["out_ids"][inside][ok])
    assert_guard(got, oo[-1])


@pytest.mark.parametrize("case", ["decreasing", "past_the_turns", "offsets_end", "offsets_start"])
def test_structures_that_do_not_fit_are_reported_and_nothing_is_written_outside(case):
    b = small_batch()
    ids, offsets, roles, conv = b.args()
    n_turns = len(roles)
    if case == "decreasing":
        conv = [0, 5, 2, 7, 8]
    elif case == "past_the_turns":
        conv = [0, 2, 5, 7, n_turns + 3]
    elif case == "offsets_end":
        offsets = offsets[:-1] + [offsets[-1] + 4]
    else:
        offsets = [1] + offsets[1:]
    got = run(TPL_BE, ids, offsets, roles, conv, loss=0b010)
    assert max(got["err"]) == _capi.E_ARG, got["err"]
    assert_guard(got, got["cap"])
    if case in ("decreasing", "past_the_turns"):  # the turns' scan does not depend on the conversations
        want = R.render(TPL_BE, *b.args(), loss_roles=0b010)
        assert np.array_equal(got["turn_offsets"], want["turn_offsets"])
        if case == "past_the_turns":  # .. and every conversation but the last is as it was
            assert np.array_equal(got["out_offsets"], want["out_offsets"])
            n = want["out_offsets"][3]
            for k in PER_TOKEN:
                assert np.array_equal(got[k][:n], want[k][:n]), k


def test_capacity():
    b = small_batch()
    want = R.render(TPL_BE, *b.args(), loss_roles=0b010)
    n_out = len(want["out_ids"])
    for cap in (n_out - 1, S - 1, S, 0):
        got = run(TPL_BE, *b.args(), loss=0b010, out_cap=cap)
        assert got["err"] == [0, _capi.E_CAPACITY]
        assert_guard(got, cap)
        assert np.array_equal(got["out_offsets"], want["out_offsets"])
    got, _ = check(TPL_BE, *b.args(), loss=0b010, out_cap=n_out)  # exactly enough
    assert got["err"] == [0, 0]


def test_no_conversations_and_no_turns():
    got, want = check(TPL_BE, [], [0], [], [0])
    assert got["out_offsets"].tolist() == [0]
    got, want = check(TPL_BE, [], [0], [], [0, 0, 0, 0])
    assert got["out_ids"][:6].tolist() == [1, 2, 1, 2, 1, 2]
    check(TPL_0, [], [0], [], [0, 0, 0], gen=0)
    check(TPL_0, [], [0], [], [0, 0, 0])  # nothing at all to write


# ---- composition: encode, render, collate, pack, spans ------------------------------------------------------------------
MARKERS = {"<|im_start|>": 50257, "<|im_end|>": 50258, "<|begin_of_text|>": 50259, "<|start_header_id|>": 50260,
           "<|end_header_id|>": 50261, "<|eot_id|>": 50262}
CONVERSATIONS = [
    [{"role": "system", "content": "You are a careful assistant."}, {"role": "user", "content": "What is 2 + 2?"},
     {"role": "assistant", "content": "2 + 2 is 4."}, {"role": "user", "content": "And twice that?"},
     {"role": "assistant", "content": "Twice that is 8, since 4 + 4 = 8."}],
    [("user", "Say <|im_end|> literally, please."), ("assistant", "")],
    [],
    [("user", "hi"), ("assistant", "Hello! How can I help you today? " * 6), ("user", "Never mind."), ("assistant", "All right.")],
    [("assistant", "An answer without a question.")],
]


@pytest.fixture(scope="module")
def vg_chat():
    import hutoken_amd
    from hutoken_amd import data
    vp, sp, kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, prefix=kw["prefix"], is_byte_encoder=kw["is_byte_encoder"], device=0)
    hutoken_amd.set_special_tokens(MARKERS)
    yield hutoken_amd
    hutoken_amd.set_special_tokens(None)


def _turns(conversation):
    return [(t["role"], t["content"]) if isinstance(t, dict) else t for t in conversation]


def enc(H, text, special=False):
    return [] if not text else H.encode_special(text) if special else H.encode(text)


def host_composition(H, preset, conversations, gen=None, special=False):
    """-> per conversation (ids, labels, text): the pieces encoded one by one on the host's side of the library"""
    if preset == "chatml":
        pre, suf, bos, n_loss = "<|im_start|>%s\n", "<|im_end|>\n", None, 1
    else:
        pre, suf, bos, n_loss = "<|start_header_id|>%s<|end_header_id|>\n\n", "<|eot_id|>", "<|begin_of_text|>", 1
    rows = []
    for c in conversations:
        ids, labels, text = [], [], ""
        if bos:
            ids += H.encode_special(bos)
            labels += [IGN]
            text += bos
        for role, content in _turns(c):
            p, s = H.encode_special(pre % role), H.encode_special(suf)
            body = enc(H, content, special)
            mine = role == "assistant"
            ids += p + body + s
            labels += [IGN] * len(p) + (body + s[:n_loss] + [IGN] * (len(s) - n_loss) if mine else [IGN] * (len(body) + len(s)))
            text += pre % role + content + suf
        if gen:
            p = H.encode_special(pre % gen)
            ids += p
            labels += [IGN] * len(p)
            text += pre % gen
        rows.append((ids, labels, text))
    return rows


def padded(rows, L, pad, truncation, side):
    out = []
    for r in rows:
        r = list(r[:L] if truncation == "right" else r[max(0, len(r) - L):])
        fill = [pad] * (L - len(r))
        out.append(r + fill if side == "right" else fill + r)
    return np.array(out, dtype=np.int64).reshape(len(rows), L)


@pytest.mark.parametrize("preset", ["chatml", "llama3"])
def test_batch_encode_chat_equals_the_host_composition(vg_chat, preset):
    import torch
    H = vg_chat
    tpl = getattr(H.ChatTemplate, preset)()
    rows = host_composition(H, preset, CONVERSATIONS)
    longest = max(len(r[0]) for r in rows)
    eot = MARKERS["<|im_end|>" if preset == "chatml" else "<|eot_id|>"]
    for max_length in (None, 40):
        L = longest if max_length is None else max_length
        for truncation in ("right", "left"):
            for side in ("right", "left"):
                for dtype in (torch.int32, torch.int64):
                    ids, mask, lengths, labels = H.batch_encode_chat(CONVERSATIONS, max_length, template=tpl, truncation=truncation,
                                                                     padding_side=side, pad_id=-7, dtype=dtype)
                    assert ids.dtype == dtype and labels.dtype == dtype and ids.shape == labels.shape == (len(rows), L)
                    assert np.array_equal(ids.cpu().numpy(), padded([r[0] for r in rows], L, -7, truncation, side))
                    assert np.array_equal(labels.cpu().numpy(), padded([r[1] for r in rows], L, IGN, truncation, side))
                    assert lengths.tolist() == [min(len(r[0]), L) for r in rows]
                    assert np.array_equal(mask.cpu().numpy() != 0, padded([[1] * len(r[0]) for r in rows], L, 0, truncation, side) != 0)
    # the labels: the assistant's content and its end-of-turn id, nothing else
    ids, mask, lengths, labels, plan = H.batch_encode_chat(CONVERSATIONS, template=tpl, return_plan=True)
    assert plan.shape == (len(rows), 8)
    ids, labels = ids.cpu().numpy(), labels.cpu().numpy()
    for i, c in enumerate(CONVERSATIONS):
        n_assistant = sum(role == "assistant" for role, _content in _turns(c))
        on = labels[i] != IGN
        assert (labels[i][on] == ids[i][on]).all() and (ids[i][on] == eot).sum() == n_assistant
        want = sum(len(enc(H, content)) + 1 for role, content in _turns(c) if role == "assistant")
        assert on.sum() == want
    # the rendered text is the template's
    for i, (row, _labels, text) in enumerate(rows):
        if row:
            assert H.decode_special(ids[i][:len(row)].tolist()) == text
    # a marker inside a user's text stays text unless asked for
    marker = MARKERS["<|im_end|>"]
    plain = sum(r[0].count(marker) for r in rows)
    sp = H.batch_encode_chat(CONVERSATIONS, template=tpl, special=True)[0].cpu().numpy()
    assert (sp == marker).sum() == plain + 1
    want = host_composition(H, preset, CONVERSATIONS, special=True)
    assert np.array_equal(sp, padded([r[0] for r in want], sp.shape[1], 0, "right", "right"))
    tpl.close()


def test_markers_that_are_not_one_id_are_named(vg_chat):
    H = vg_chat
    H.set_special_tokens({k: v for k, v in MARKERS.items() if k != "<|eot_id|>"})
    try:
        with pytest.raises(ValueError, match=r"<\|eot_id\|>"):
            H.ChatTemplate.llama3()
        H.ChatTemplate.chatml().close()
        H.set_special_tokens({k: v for k, v in MARKERS.items() if k != "<|im_start|>"})
        with pytest.raises(ValueError, match=r"<\|im_start\|>"):
            H.ChatTemplate.chatml()
    finally:
        H.set_special_tokens(MARKERS)


def test_generation_prompt(vg_chat):
    H = vg_chat
    tpl = H.ChatTemplate.chatml()
    rows = host_composition(H, "chatml", CONVERSATIONS, gen="assistant")
    ids, mask, lengths, labels = H.batch_encode_chat(CONVERSATIONS, template=tpl, add_generation_prompt="assistant", pad_id=-7)
    ids, labels = ids.cpu().numpy(), labels.cpu().numpy()
    head = H.encode_special("<|im_start|>assistant\n")
    for i, (row, lab, _text) in enumerate(rows):
        n = int(lengths[i])
        assert n == len(row) and ids[i][:n].tolist() == row and labels[i][:n].tolist() == lab
        assert ids[i][n - len(head):n].tolist() == head and (labels[i][n - len(head):] == IGN).all()
    tpl.close()


def test_two_packers_give_aligned_rows(vg_chat):
    """The rendered pair goes through SequencePacker as the encode's does; a second packer of the same geometry, fed the
    labels along the same offsets, gives the label rows."""
    import torch
    H = vg_chat
    tpl = H.ChatTemplate.llama3()
    contents, roles, conv = H._chat_turns(CONVERSATIONS * 7, tpl)
    dev = torch.device("cuda", 0)
    ids, oo = H._texts_to_device(contents)
    out_ids, out_offsets, labels = H.render_chat_device(ids, oo, torch.tensor(conv, device=dev), torch.tensor(roles, dtype=torch.int32, device=dev),
                                                        tpl, check=True)
    L = 32
    with H.SequencePacker(L) as p_ids, H.SequencePacker(L, pad_id=IGN) as p_lab:
        a, b = p_ids.add(out_ids, out_offsets, check=True), p_lab.add(labels, out_offsets, check=True)
        ta, tb = p_ids.flush(), p_lab.flush()
    rows = host_composition(H, "llama3", CONVERSATIONS * 7)
    flat_ids, flat_lab = sum((r[0] for r in rows), []), sum((r[1] for r in rows), [])
    n = len(flat_ids) // L * L
    assert a["input_ids"].shape == b["input_ids"].shape == (n // L, L)
    assert a["input_ids"].cpu().numpy().ravel().tolist() == flat_ids[:n]
    assert b["input_ids"].cpu().numpy().ravel().tolist() == flat_lab[:n]
    for k in ("position_ids", "segment_ids"):
        assert torch.equal(a[k], b[k]) and torch.equal(ta[k], tb[k])
    rest = len(flat_ids) - n
    assert ta["input_ids"].shape[0] == tb["input_ids"].shape[0] == (1 if rest else 0)
    if rest:
        assert ta["input_ids"][0, :rest].tolist() == flat_ids[n:] and tb["input_ids"][0, :rest].tolist() == flat_lab[n:]
        assert (tb["input_ids"][0, rest:] == IGN).all()
    tpl.close()


def test_token_spans_are_carried_over_by_the_source(vg_chat):
    """token_spans_device over the turns' texts, indexed by `source`: every content token of the rendered stream gets the
    span it has in its own turn's text."""
    import torch
    H = vg_chat
    tpl = H.ChatTemplate.chatml()
    contents, roles, conv = H._chat_turns(CONVERSATIONS, tpl)
    dev = torch.device("cuda", 0)
    ids, oo, d_bytes, d_offs = H._texts_to_device(contents, with_text=True)
    spans = H.token_spans_device(d_bytes, d_offs, ids, oo, unit="char")
    out_ids, out_offsets, labels, turn_ids, source = H.render_chat_device(
        ids, oo, torch.tensor(conv, device=dev), torch.tensor(roles, dtype=torch.int32, device=dev), tpl,
        return_turn_ids=True, return_source=True, check=True)
    n_out = int(out_offsets[-1])
    source, turn_ids, out_ids = source[:n_out], turn_ids[:n_out], out_ids[:n_out].cpu().numpy()
    content = source >= 0
    carried = spans[source[content]].cpu().numpy()
    host_ids, host_spans = H.batch_encode_with_offsets(contents, unit="char")
    assert carried.tolist() == [list(s) for row in host_spans for s in row]
    assert out_ids[content.cpu().numpy()].tolist() == [t for row in host_ids for t in row]
    # .. and the turn a token belongs to names the text its span is in
    oo_host, src, tid = out_offsets.cpu().numpy(), source.cpu().numpy(), turn_ids.cpu().numpy()
    turn_of_id = np.repeat(np.arange(len(contents)), np.diff(oo.cpu().numpy()))
    spans_host = spans.cpu().numpy()
    for i in range(len(conv) - 1):
        for k in range(oo_host[i], oo_host[i + 1]):
            if src[k] >= 0:
                t = turn_of_id[src[k]]
                assert t == conv[i] + tid[k]
                a, b = spans_host[src[k]].tolist()
                assert 0 <= a <= b <= len(contents[t])
    tpl.close()
