"""Fill-in-the-middle without a GPU: the worked example by hand, the two functions of csrc/hutk_fim.h (through their debug
exports) against the rule's restatement (fim_ref), the shares the draw gives, the bound, the exports, the Python
argument checks and everything the C ABI refuses before it looks for a device."""
import itertools
import random

import numpy as np
import pytest

import fim_ref as R
import hutoken_amd as H
from hutoken_amd import _capi

NO = _capi.NO_TOKEN
IGN = -100
ONE = 2**32


def test_names_are_exported():
    for name in ("fim_device", "fim_cut_text_device", "fim_pieces_device", "batch_encode_fim"):
        assert name in H.__all__ and callable(getattr(H, name)) and name in H.__doc__
    lib = _capi.load()
    for name in ("hutk_fim_ids_bound", "hutk_fim_cut_text_device", "hutk_fim_plan_tokens_device", "hutk_fim_plan_pieces_device",
                 "hutk_fim_render_device", "hutk_debug_fim_span", "hutk_debug_fim_decide", "hutk_debug_fim_locate"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert _capi.fim_span() >= 256 and _capi.fim_span() % 256 == 0
    assert _capi.FIM_PARTS.index("sentinel") == R.PART_SENTINEL and _capi.FIM_PARTS.index("middle") == R.PART_MIDDLE
    assert (_capi.FIM_PLAIN, _capi.FIM_PSM, _capi.FIM_SPM) == (R.PLAIN, R.PSM, R.SPM)


# ---- the worked example ------------------------------------------------------------------------------------------------
def test_worked_example():
    x = [10, 11, 12, 13, 14]
    plan = [[0, 5, 1, 3]]
    r = R.render(x, plan, [R.PSM], pre=1, suf=2, mid=3, end=4)
    assert r["out_ids"].tolist() == [1, 10, 2, 13, 14, 3, 11, 12, 4]
    assert r["source"].tolist() == [-1, 0, -1, 3, 4, -1, 1, 2, -1]
    assert r["parts"].tolist() == [4, 1, 4, 3, 3, 4, 2, 2, 4]
    r = R.render(x, plan, [R.SPM], pre=1, suf=2, mid=3, end=4, loss_parts=R.LOSS_MIDDLE)
    assert r["out_ids"].tolist() == [1, 2, 13, 14, 3, 10, 11, 12, 4]
    assert r["source"].tolist() == [-1, -1, 3, 4, -1, 0, 1, 2, -1]
    assert r["labels"].tolist() == [IGN] * 6 + [11, 12, 4]
    r = R.render(x, plan + [[5, 0, 0, 0]], [R.PLAIN, R.PSM], pre=1, suf=2, mid=3)
    assert r["out_ids"].tolist() == x + [1, 2, 3] and r["out_offsets"].tolist() == [0, 5, 8]
    assert r["parts"].tolist() == [0] * 5 + [4] * 3
    # the same through the library's two functions
    for kind, want in ((R.PSM, [1, 10, 2, 13, 14, 3, 11, 12, 4]), (R.SPM, [1, 2, 13, 14, 3, 10, 11, 12, 4])):
        got = []
        for p in range(9):
            part, v = _capi.fim_locate(5, 1, 3, kind, True, p)
            got.append((1, 2, 3, 4)[v] if part == R.PART_SENTINEL else x[v])
        assert got == want
        assert _capi.fim_locate(5, 1, 3, kind, True, 9) == (-1, -1) and _capi.fim_locate(5, 1, 3, kind, False, 8) == (-1, -1)


# ---- hutk_fim.h against the restatement ----------------------------------------------------------------------------------
def test_decide_matches_the_restatement():
    rng = random.Random(4)
    cases = []
    lens = [0, 1, 2, 3, 7, 100, 65535, 2**31 - 1, 2**31, 2**31 + 5, 2**40]
    docs = [0, 1, 2**32 - 1, 2**32, 2**32 + 17, 2**40 + 3, 2**62]
    seeds = [0, 7, 1234, 2**32, 2**64 - 1]
    thresholds = [(0, 0), (ONE, ONE), (ONE, 0), (0, ONE), (ONE // 2, ONE // 2), (ONE // 10, ONE - 1), (1, 1)]
    for seed, doc, length in itertools.product(seeds, docs, lens):
        cases.append((seed, doc, length) + rng.choice(thresholds))
    for _ in range(3000):
        cases.append((rng.randrange(2**64), rng.randrange(2**62), rng.choice((rng.randrange(0, 50), rng.randrange(0, 2**31))))
                     + rng.choice(thresholds))
    assert len(cases) > 3000
    kinds = set()
    for seed, doc, length, fb, sb in cases:
        kind, lo, hi = (int(v) for v in R.decide(seed, doc, length, fb, sb))
        assert _capi.fim_decide(seed, doc, length, fb, sb) == (kind, lo, hi), (seed, doc, length, fb, sb)
        assert 0 <= lo <= hi <= length
        if fb == 0 or length < 1 or length >= 2**31:
            assert (kind, lo, hi) == (R.PLAIN, length, length)
        if fb == ONE and 1 <= length < 2**31:
            assert kind == (R.SPM if sb == ONE else R.PSM if sb == 0 else kind) and kind != R.PLAIN
        kinds.add(kind)
    assert kinds == {R.PLAIN, R.PSM, R.SPM}
    lib = _capi.load()
    out = (_capi._i64 * 3)()
    for fb, sb in ((-1, 0), (0, -1), (ONE + 1, 0), (0, ONE + 1)):
        assert lib.hutk_debug_fim_decide(1, 0, 5, fb, sb, out) == _capi.E_ARG
    assert lib.hutk_debug_fim_decide(1, 0, 5, 0, 0, None) == _capi.E_ARG


def test_locate_every_position_of_small_documents():
    for n in range(13):
        for lo in range(n + 1):
            for hi in range(lo, n + 1):
                for kind, E in itertools.product((R.PLAIN, R.PSM, R.SPM), (0, 1)):
                    want = R.layout(n, lo, hi, kind, E)
                    assert len(want) == R.rendered_length(n, kind, E)
                    got = [_capi.fim_locate(n, lo, hi, kind, E, p) for p in range(len(want))]
                    assert got == want, (n, lo, hi, kind, E)
                    assert _capi.fim_locate(n, lo, hi, kind, E, len(want))[0] == -1
                    assert _capi.fim_locate(n, lo, hi, kind, E, -1)[0] == -1
                    # a permutation of the document's ids plus exactly 3 + E sentinels (none in a plain document)
                    assert sorted(v for part, v in got if part != R.PART_SENTINEL) == list(range(n))
                    sentinels = [v for part, v in got if part == R.PART_SENTINEL]
                    assert sorted(sentinels) == ([] if kind == R.PLAIN else list(range(3 + E)))
                    for part, v in got:
                        if part == R.PART_PREFIX:
                            assert v < lo
                        elif part == R.PART_MIDDLE:
                            assert lo <= v < hi
                        elif part == R.PART_SUFFIX:
                            assert hi <= v
    lib = _capi.load()
    out = (_capi._i64 * 2)()
    for args in ((5, 3, 2, 1, 0, 0), (5, -1, 2, 1, 0, 0), (5, 1, 6, 1, 0, 0), (5, 1, 2, 3, 0, 0), (5, 1, 2, -1, 0, 0)):
        assert lib.hutk_debug_fim_locate(*args, out) == _capi.E_ARG
    assert lib.hutk_debug_fim_locate(5, 1, 2, 1, 0, 0, None) == _capi.E_ARG


@pytest.mark.parametrize("seed", [1234, 7])
def test_shares_of_the_draw(seed):
    """20000 documents of length 100 at fim_rate = spm_rate = 0.5: the transformed share and the SPM share among them
    within 0.5 +- 0.02 (four standard deviations of a share of 20000, resp. of about 10000, draws: 4 * 0.0035 = 0.014,
    4 * 0.005 = 0.02), the mean middle length within 33.7 +- 1.5 (|a - b| of two uniform draws from 0 .. 100 has mean
    33.66 and standard deviation 23.8: four standard deviations of the mean of 10000 are 0.95).  The restatement gives
    0.5000 / 0.4997 for seed 1234 and 0.4979 / 0.4982 for seed 7; the mean middle is 34.19 resp. 33.45 among the
    transformed documents, and 33.85 resp. 33.63 over the cuts of all 20000 draws (the same documents at fim_rate 1)."""
    kind, lo, hi = R.decide(seed, np.arange(20000), 100, ONE // 2, ONE // 2)
    t = kind != R.PLAIN
    share, spm, middle = t.mean(), (kind[t] == R.SPM).mean(), (hi - lo)[t].mean()
    _k, lo_all, hi_all = R.decide(seed, np.arange(20000), 100, ONE, ONE // 2)
    assert (lo_all[t] == lo[t]).all() and (hi_all[t] == hi[t]).all()  # (the cuts do not depend on the rates)
    middle_all = (hi_all - lo_all).mean()
    print("seed %d: transformed %.4f, SPM among them %.4f, mean middle %.2f (of all draws %.2f)" % (seed, share, spm, middle, middle_all))
    assert abs(share - 0.5) <= 0.02
    assert abs(spm - 0.5) <= 0.02
    assert abs(middle - 33.7) <= 1.5
    assert abs(middle_all - 33.7) <= 1.5
    # and the library draws the same
    for d in range(0, 20000, 97):
        assert _capi.fim_decide(seed, d, 100, ONE // 2, ONE // 2) == (int(kind[d]), int(lo[d]), int(hi[d]))


# ---- the bound -------------------------------------------------------------------------------------------------------
def test_ids_bound():
    lib = _capi.load()
    assert lib.hutk_fim_ids_bound(0, 0, 0) == 0 and lib.hutk_fim_ids_bound(0, 0, 1) == 0
    assert lib.hutk_fim_ids_bound(10, 1000, 0) == 1030 and lib.hutk_fim_ids_bound(10, 1000, 1) == 1040
    assert lib.hutk_fim_ids_bound(2**31 - 2, 2**40, 1) == 2**40 + 4 * (2**31 - 2)
    for args in ((-1, 0, 0), (0, -1, 0), (2**31 - 1, 0, 0)):
        assert lib.hutk_fim_ids_bound(*args) == -_capi.E_ARG
    with pytest.raises(TypeError):
        _capi.fim_ids_bound(-1, 0, False)
    # it holds, and is the length when every document is transformed
    rng = random.Random(9)
    for trial in range(40):
        offsets = np.cumsum([0] + [rng.randrange(0, 9) for _ in range(rng.randrange(0, 12))])
        ids = np.arange(100, 100 + offsets[-1])
        end = rng.choice((None, 4))
        rate = rng.choice((0, ONE // 2, ONE))
        r = R.fim_tokens(ids, offsets, seed=trial, fim_below=rate, spm_below=ONE // 2, pre=1, suf=2, mid=3, end=end)
        bound = lib.hutk_fim_ids_bound(len(offsets) - 1, len(ids), end is not None)
        assert bound >= len(r["out_ids"]) == r["out_offsets"][-1]
        if rate == ONE and all(offsets[i + 1] > offsets[i] for i in range(len(offsets) - 1)):
            assert bound == len(r["out_ids"])
        if rate == 0:
            assert r["out_ids"].tolist() == ids.tolist() and r["out_offsets"].tolist() == offsets.tolist()


# ---- the text cut's restatement -------------------------------------------------------------------------------------------
def test_cut_text_restatement_keeps_characters_whole():
    texts = ["plain ascii text", "", "árvíztűrő tükörfúrógép", "日本語のテキスト", "🙂🙃🙂🙃", "a"]
    data = b"".join(t.encode() for t in texts)
    offsets = np.cumsum([0] + [len(t.encode()) for t in texts])
    for seed in range(50):
        pieces, kinds = R.cut_text(data, offsets, seed=seed, fim_below=ONE, spm_below=ONE // 2)
        assert pieces[-1] == len(data) and (np.diff(pieces) >= 0).all()
        for i, t in enumerate(texts):
            parts = [data[pieces[3 * i + k]:pieces[3 * i + k + 1]].decode() for k in range(3)]  # each decodes
            assert "".join(parts) == t
            assert kinds[i] == (R.PLAIN if not t else kinds[i]) and (t == "" or kinds[i] != R.PLAIN)
    pieces, kinds = R.cut_text(data, offsets, seed=1, fim_below=0, spm_below=0)
    assert (kinds == 0).all() and pieces[1::3].tolist() == offsets[1:].tolist() and pieces[2::3].tolist() == offsets[1:].tolist()
    assert R.char_start(b"a" + b"\x80" * 5, 5) == 2  # at most three steps back
    assert R.char_start(b"\x80\x80", 1) == 0 and R.char_start(b"ab", 2) == 2 and R.char_start(b"ab", 0) == 0


# ---- the Python argument checks ----------------------------------------------------------------------------------------
def test_python_argument_checks():
    import torch
    ids = torch.zeros(4, dtype=torch.int32)
    offs = torch.tensor([0, 2, 4], dtype=torch.int64)
    sent = dict(prefix_id=1, suffix_id=2, middle_id=3)
    with pytest.raises(TypeError, match="seed"):
        H.fim_device(ids, offs, **sent)                                   # seed has no default
    for name in sent:
        with pytest.raises(TypeError, match=name):
            H.fim_device(ids, offs, seed=1, **dict(sent, **{name: None}))
        with pytest.raises(ValueError, match=name):
            H.fim_device(ids, offs, seed=1, **dict(sent, **{name: 2**31}))
    with pytest.raises(TypeError, match="end_id"):
        H.fim_device(ids, offs, seed=1, end_id="4", **sent)
    with pytest.raises(TypeError, match="seed must be an int"):
        H.fim_device(ids, offs, seed=1.0, **sent)
    with pytest.raises(ValueError, match="seed"):
        H.fim_device(ids, offs, seed=-1, **sent)
    for name in ("fim_rate", "spm_rate"):
        with pytest.raises(ValueError, match=name):
            H.fim_device(ids, offs, seed=1, **dict(sent, **{name: 1.5}))
        with pytest.raises(TypeError, match=name):
            H.fim_device(ids, offs, seed=1, **dict(sent, **{name: "0.5"}))
    with pytest.raises(TypeError, match="first_doc"):
        H.fim_device(ids, offs, seed=1, first_doc=1.0, **sent)
    with pytest.raises(ValueError, match="first_doc"):
        H.fim_device(ids, offs, seed=1, first_doc=-1, **sent)
    for bad in ("prefix", 5, None, ("middle", "tail")):
        with pytest.raises(ValueError, match="loss_on"):
            H.fim_device(ids, offs, seed=1, loss_on=bad, **sent)
    assert H._fim_loss_arg("all") == R.LOSS_ALL and H._fim_loss_arg("middle") == R.LOSS_MIDDLE
    assert H._fim_loss_arg(("prefix", "suffix")) == 0b1010 and H._fim_loss_arg(()) == 0 and H._fim_loss_arg(["end"]) == R.LOSS_END
    with pytest.raises(TypeError, match="ignore_index"):
        H.fim_device(ids, offs, seed=1, ignore_index=1.0, **sent)
    with pytest.raises(ValueError, match="ignore_index"):
        H.fim_device(ids, offs, seed=1, ignore_index=2**31, **sent)
    for name in ("return_labels", "return_parts", "return_source", "check"):
        with pytest.raises(TypeError, match=name):
            H.fim_device(ids, offs, seed=1, **dict(sent, **{name: 1}))
    with pytest.raises(TypeError, match="ids must be a torch tensor"):
        H.fim_device([1, 2], offs, seed=1, **sent)
    with pytest.raises(TypeError, match="offsets must have dtype int64"):
        H.fim_device(ids, offs.to(torch.int32), seed=1, **sent)
    with pytest.raises(ValueError, match="at least one entry"):
        H.fim_device(ids, offs[:0], seed=1, **sent)
    with pytest.raises(ValueError, match="must be on the GPU"):
        H.fim_device(ids, offs, seed=1, **sent)
    # the pieces form
    kinds = torch.zeros(1, dtype=torch.int32)
    offs3 = torch.tensor([0, 1, 2, 4], dtype=torch.int64)
    with pytest.raises(TypeError, match="seed"):
        H.fim_pieces_device(ids, offs3, kinds, seed=1, **sent)            # nothing is drawn there
    with pytest.raises(TypeError, match="kinds must have dtype int32"):
        H.fim_pieces_device(ids, offs3, kinds.to(torch.int64), **sent)
    with pytest.raises(ValueError, match="3 n_docs \\+ 1"):
        H.fim_pieces_device(ids, offs, kinds, **sent)
    with pytest.raises(ValueError, match="one entry per document"):
        H.fim_pieces_device(ids, offs3, torch.zeros(2, dtype=torch.int32), **sent)
    with pytest.raises(ValueError, match="loss_on"):
        H.fim_pieces_device(ids, offs3, kinds, loss_on="x", **sent)
    with pytest.raises(ValueError, match="must be on the GPU"):
        H.fim_pieces_device(ids, offs3, kinds, **sent)
    # the text cut
    data = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(TypeError, match="seed"):
        H.fim_cut_text_device(data, offs)
    with pytest.raises(ValueError, match="fim_rate"):
        H.fim_cut_text_device(data, offs, seed=1, fim_rate=-0.1)
    with pytest.raises(TypeError, match="check"):
        H.fim_cut_text_device(data, offs, seed=1, check=1)
    with pytest.raises(TypeError, match="d_bytes must have dtype uint8"):
        H.fim_cut_text_device(ids, offs, seed=1)
    with pytest.raises(ValueError, match="must be on the GPU"):
        H.fim_cut_text_device(data, offs, seed=1)
    # the list form: everything is checked before anything is encoded (no context is initialised here)
    with pytest.raises(TypeError, match="seed"):
        H.batch_encode_fim(["a"], **sent)
    with pytest.raises(TypeError, match="prefix_id"):
        H.batch_encode_fim(["a"], seed=1, prefix_id=None, suffix_id=2, middle_id=3)
    with pytest.raises(ValueError, match="level"):
        H.batch_encode_fim(["a"], seed=1, level="word", **sent)
    with pytest.raises(ValueError, match="loss_on"):
        H.batch_encode_fim(["a"], seed=1, loss_on="assistant", **sent)
    with pytest.raises(ValueError, match="dtype"):
        H.batch_encode_fim(["a"], seed=1, dtype="int16", **sent)
    with pytest.raises(ValueError, match="spm_rate"):
        H.batch_encode_fim(["a"], seed=1, spm_rate=2, **sent)


# ---- the C ABI: what is refused before a device is looked for ---------------------------------------------------------
P = 256  # an address that is never read: every check below comes before a device is looked for


def cut_call(n_docs=3, n_bytes=10, seed=1, first=0, fb=ONE // 2, sb=ONE // 2, data=P, offs=P, pieces=P, kinds=P, err=None):
    return _capi.load().hutk_fim_cut_text_device(data, offs, n_docs, n_bytes, seed, first, fb, sb, pieces, kinds, err, None)


def tokens_call(n_docs=3, n_ids=10, seed=1, first=0, fb=ONE // 2, sb=ONE // 2, end=1, offs=P, oo=P, plan=P, kinds=P, err=None):
    return _capi.load().hutk_fim_plan_tokens_device(offs, n_docs, n_ids, seed, first, fb, sb, end, oo, plan, kinds, err, None)


def pieces_call(n_docs=3, n_ids=10, end=1, offs=P, kinds=P, oo=P, plan=P, err=None):
    return _capi.load().hutk_fim_plan_pieces_device(offs, kinds, n_docs, n_ids, end, oo, plan, err, None)


def render_call(n_docs=3, n_ids=10, pre=1, suf=2, mid=3, end=NO, loss=31, cap=64, ids=P, plan=P, kinds=P, oo=P, out=P,
                labels=None, parts=None, src=None, err=None):
    return _capi.load().hutk_fim_render_device(ids, plan, kinds, oo, n_docs, n_ids, pre, suf, mid, end, loss, IGN, cap, out,
                                               labels, parts, src, err, None)


def good(call, **kw):
    """The same call with good arguments reaches the device question: HUTK_E_DEVICE on a machine without a GPU.  (With
    one it would run on addresses that are none, so there it is not made.)"""
    import torch
    return torch.cuda.is_available() or call(**kw) == _capi.E_DEVICE


def test_device_calls_are_checked_before_a_device_is_looked_for():
    E = _capi.E_ARG
    calls = (cut_call, tokens_call, pieces_call, render_call)
    for call in calls:                                                    # the same calls with good arguments
        assert good(call)
        assert good(call, err=P)
        for kw in ({"n_docs": -1}, {"n_docs": 2**31 - 1}, {"n_ids" if call is not cut_call else "n_bytes": -1}):
            assert call(**kw) == E, (call.__name__, kw)
        assert call(err=P + 2) == E
    assert "n_docs below 2^31 - 1" in _capi.last_error() or "aligned" in _capi.last_error()
    for call in (cut_call, tokens_call):
        for kw in ({"fb": -1}, {"fb": ONE + 1}, {"sb": -1}, {"sb": ONE + 1}, {"first": -1}, {"first": 2**63 - 1}):
            assert call(**kw) == E, (call.__name__, kw)
        for kw in ({"fb": 0, "sb": 0}, {"fb": ONE, "sb": ONE}, {"first": 2**40}, {"seed": 2**64 - 1}):
            assert good(call, **kw)
    # NULL or misaligned required buffers, with work to do
    for call, names in ((cut_call, ("data", "offs", "pieces", "kinds")), (tokens_call, ("offs", "oo", "plan", "kinds")),
                        (pieces_call, ("offs", "kinds", "oo", "plan")), (render_call, ("ids", "plan", "kinds", "oo", "out"))):
        for name in names:
            assert call(**{name: None}) == E, (call.__name__, name)
            if name != "data":
                assert call(**{name: P + 2}) == E, (call.__name__, name)
    assert good(cut_call, data=None, n_bytes=0) and good(cut_call, data=P + 1)
    assert good(render_call, ids=None, n_ids=0) and good(render_call, out=None, cap=0)
    assert good(render_call, ids=P + 4, out=P + 4, labels=P + 12, parts=P + 8, src=P + 8, plan=P + 8, oo=P + 8, kinds=P + 4)
    for name in ("labels", "parts", "src"):
        assert good(render_call, **{name: P}) and render_call(**{name: P + 2}) == E
    assert render_call(src=P + 4) == E
    # without documents there is no work: only out_offsets (the piece offsets) is needed
    assert good(tokens_call, n_docs=0, n_ids=0, offs=None, plan=None, kinds=None)
    assert tokens_call(n_docs=0, n_ids=0, offs=None, plan=None, kinds=None, oo=None) == E
    assert good(pieces_call, n_docs=0, n_ids=0, offs=None, plan=None, kinds=None)
    assert pieces_call(n_docs=0, n_ids=0, offs=None, plan=None, kinds=None, oo=None) == E
    assert good(cut_call, n_docs=0, n_bytes=0, data=None, offs=None, kinds=None)
    assert cut_call(n_docs=0, n_bytes=0, data=None, offs=None, kinds=None, pieces=None) == E
    assert cut_call(n_docs=0, n_bytes=5) == E
    assert good(render_call, n_docs=0, n_ids=0, ids=None, plan=None, kinds=None, oo=None, out=None)
    # the render's own
    for name in ("pre", "suf", "mid"):
        assert render_call(**{name: NO}) == E
    assert "HUTK_NO_TOKEN" in _capi.last_error()
    assert good(render_call, end=4) and good(render_call, end=NO)
    for loss in (64, 1 << 15, 1 << 31):
        assert render_call(loss=loss) == E
    for loss in (0, 31, 32, 63):
        assert good(render_call, loss=loss)
    assert render_call(cap=-1) == E


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.fim_plan_tokens_device(P, 1, 1, 1, 0, 0, 0, False, P, P, P)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.fim_render_device(P, P, P, P, 1, 1, 1, 2, 3, NO, 31, IGN, 8, P)
    with pytest.raises(RuntimeError, match="no HIP device"):
        _capi.fim_cut_text_device(P, P, 1, 1, 1, 0, 0, 0, P, P)
