"""Row-aligned features on the GPU (csrc/hutk_collate.hip: k_plan_*, k_rows_gather, k_rows_answers; csrc/hutk_features.hip:
k_word_ids) against the plain restatement of tests/features_ref.py, every comparison exact and over every element.

The ids are the GPU's own (VG with the gpt2 and cl100k presets); their byte and character spans come from spans_ref with
the oracle's per-token decoding, the word starts from presplit_ref.  tests/test_features_cpu.py confirms on the CPU that
the texts used here give no unknown ids and no span mismatches.  Needs a real MI355X."""
import functools

import numpy as np
import pytest

import features_cases as FC
import features_ref as F
import presplit_ref as SR
import spans_ref as S

pytestmark = pytest.mark.gpu

E_ARG, E_UNSUPPORTED = 4, 6
PRESETS = ("gpt2", "cl100k")
TPL = dict(bos_id=50256, sep_ids=(50255, 50254), eos_id=50253)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def host(t):
    return t.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def ragged(lens, rng, base=0):
    offs = np.full(len(lens) + 1, base, dtype=np.int64)
    offs[1:] += np.cumsum(lens, dtype=np.int64)
    return rng.integers(0, 60000, size=int(offs[-1])).astype(np.int32), offs


# ---- plans ------------------------------------------------------------------------------------------------------------
def check_plan(got, plan_ref, ids_a, ids_b, L, tpl, base):
    """A collate call with return_plan=True against the same call without and the restated plan; the plan rebuilds the
    call's own input_ids."""
    assert len(got) == len(base) + 1 and all(same(host(g), host(b)) for g, b in zip(got, base))
    plan = host(got[-1])
    assert same(plan, plan_ref), (plan[:5], plan_ref[:5])
    assert same(F.rebuild(plan, L, ids_a, ids_b, pad_id=-9, **tpl), host(got[0]))


@pytest.mark.parametrize("side", ["right", "left"])
def test_padded_plans(side):
    import hutoken_amd
    rng = np.random.default_rng(1)
    for L, tpl in ((8, {}), (7, {"bos_id": 1, "eos_id": 2}), (16, {"eos_id": 2})):
        C = L - len(tpl)
        ids, offs = ragged([0, C, C + 1, 1, 2 * C, C - 1] + list(rng.integers(0, 3 * L, size=294)), rng)
        d_ids, d_offs = dev(ids), dev(offs)
        for tr in ("right", "left"):
            kw = dict(truncation=tr, padding_side=side, pad_id=-9, check=True, **tpl)
            base = hutoken_amd.collate_padded(d_ids, d_offs, L, **kw)
            got = hutoken_amd.collate_padded(d_ids, d_offs, L, return_plan=True, **kw)
            check_plan(got, F.padded_plan(offs, L, truncation=tr, padding_side=side, **tpl), ids, None, L, tpl, base)
    # no documents: no rows
    got = hutoken_amd.collate_padded(dev(np.zeros(0, np.int32)), dev(np.zeros(1, np.int64)), 8, return_plan=True, check=True)
    assert got[-1].shape == (0, 8) and got[0].shape == (0, 8)


@pytest.mark.parametrize("side", ["right", "left"])
def test_windows_plans(side):
    import hutoken_amd
    rng = np.random.default_rng(2)
    for L, tpl in ((8, {}), (9, {"bos_id": 1, "eos_id": 2}), (33, {"bos_id": 1})):
        C = L - len(tpl)
        ids, offs = ragged([0, C, C + 1, 1, 5 * C, 0, 0, 2 * C + 1] + list(rng.integers(0, 4 * L, size=300)), rng)
        d_ids, d_offs = dev(ids), dev(offs)
        for stride in (0, C - 1, C // 2):
            kw = dict(padding_side=side, pad_id=-9, check=True, **tpl)
            base = hutoken_amd.collate_windows(d_ids, d_offs, L, stride, **kw)
            plan_ref = F.windows_plan(offs, L, stride, padding_side=side, **tpl)
            assert len(plan_ref) > 256  # more than one workgroup of the planner
            got = hutoken_amd.collate_windows(d_ids, d_offs, L, stride, return_plan=True, **kw)
            check_plan(got, plan_ref, ids, None, L, tpl, base)
            assert same(host(got[3]), plan_ref[:, :2])  # (item, start) is row_map
            got = hutoken_amd.collate_windows(d_ids, d_offs, L, stride, return_plan=True, n_ids=len(ids), n_rows=len(plan_ref), **kw)
            check_plan(got, plan_ref, ids, None, L, tpl, base)


@pytest.mark.parametrize("side", ["right", "left"])
def test_pair_plans(side):
    import hutoken_amd
    rng = np.random.default_rng(3)
    for L, tpl in ((12, {}), (16, dict(bos_id=1, sep_ids=(4, 5), eos_id=2)), (9, dict(sep_ids=(4,)))):
        R = L - (("bos_id" in tpl) + len(tpl.get("sep_ids", ())) + ("eos_id" in tpl))
        # na + nb at R, R + 1 and 2 R, either side the longer one, empty sides, one side alone above R
        lens = [(R // 2, R - R // 2), (R // 2, R - R // 2 + 1), (R - R // 2 + 1, R // 2), (R, R), (0, 2 * R), (2 * R, 0), (0, 0),
                (R + 3, 1), (1, R + 3), (R, 0), (0, R), (R - 1, 1), (1, R), (3 * R, 3 * R), (R, 5 * R + 1), (5 * R + 1, R)]
        lens += [tuple(x) for x in rng.integers(0, 2 * L, size=(290, 2))]
        a, oa = ragged([x for x, _ in lens], rng, base=3)
        b, ob = ragged([y for _, y in lens], rng)
        d = dev(a), dev(oa), dev(b), dev(ob)
        for strategy in ("longest_first", "only_first", "only_second"):
            kw = dict(truncation=strategy, padding_side=side, pad_id=-9, check=True, **tpl)
            base = hutoken_amd.collate_pairs(*d, L, **kw)
            got = hutoken_amd.collate_pairs(*d, L, return_plan=True, **kw)
            check_plan(got, F.pairs_plan(oa, ob, L, strategy, padding_side=side, **tpl), a, b, L, tpl, base)
            if strategy == "longest_first":
                continue
            for stride in (0, R - 1, 2):  # (C == 0 for the pairs whose kept side fills the row)
                base = hutoken_amd.collate_pair_windows(*d, L, stride, **kw)
                plan_ref = F.pair_windows_plan(oa, ob, L, stride, strategy, padding_side=side, **tpl)
                assert len(plan_ref) > 256
                got = hutoken_amd.collate_pair_windows(*d, L, stride, return_plan=True, **kw)
                check_plan(got, plan_ref, a, b, L, tpl, base)
                assert same(host(got[4]), plan_ref[:, :2])
                got = hutoken_amd.collate_pair_windows(*d, L, stride, return_plan=True, n_rows=len(plan_ref), **kw)
                check_plan(got, plan_ref, a, b, L, tpl, base)


def test_plans_of_offsets_that_do_not_describe_the_ids_are_empty():
    import hutoken_amd
    rng = np.random.default_rng(4)
    ids, offs = ragged(list(rng.integers(0, 20, size=50)), rng)
    bad = offs.copy()
    bad[-1] += 1  # the ends do not fit: every row is planned empty
    with pytest.raises(ValueError, match="collate_padded"):
        hutoken_amd.collate_padded(dev(ids), dev(bad), 8, n_ids=len(ids), return_plan=True, check=True)
    plan = host(hutoken_amd.collate_padded(dev(ids), dev(bad), 8, n_ids=len(ids), return_plan=True)[-1])
    assert not plan[:, [3, 6]].any() and np.array_equal(plan[:, 0], np.arange(50))
    bad = offs.copy()
    bad[20] = bad[19] - 1  # one decreasing pair: that document's row is empty, the others stay
    plan = host(hutoken_amd.collate_padded(dev(ids), dev(bad), 8, return_plan=True)[-1])
    want = F.padded_plan(offs, 8)
    assert plan[19, 3] == 0 and same(np.delete(plan, [19, 20], axis=0), np.delete(want, [19, 20], axis=0))


# ---- the gather -------------------------------------------------------------------------------------------------------
def value_arrays(n, rng):
    """the four record kinds: (values, fill) with 4, 8, 8 and 16 bytes a record"""
    return [(rng.integers(-2**31, 2**31, size=n).astype(np.int32), -1),
            (rng.integers(-2**62, 2**62, size=n).astype(np.int64), -2**40),
            (rng.integers(-2**31, 2**31, size=(n, 2)).astype(np.int32), (0, -7)),
            (rng.integers(-2**62, 2**62, size=(n, 2)).astype(np.int64), (2**40, -1))]


@pytest.mark.parametrize("L", [5, 7, 8, 512, 4100, 8192])
def test_gather_every_record_size(L):
    """5 and 7: a record per thread; 8 and 512: 16 bytes per thread, several rows per workgroup; 4100 and 8192: the column
    chunks of one long row.  300 rows are more than one workgroup holds (256 at most)."""
    import hutoken_amd
    rng = np.random.default_rng(L)
    n = 300 if L <= 512 else 3
    lens = [0, L, L + 1, 1] + list(rng.integers(0, 2 * L if L <= 512 else L + 50, size=n - 4)) if n > 3 else [L + 5, 0, L - 3]
    ids, offs = ragged(lens, rng)
    d_ids, d_offs = dev(ids), dev(offs)
    for side in ("right", "left"):
        # one side: padded rows, cut on the left
        plan_t = hutoken_amd.collate_padded(d_ids, d_offs, L, bos_id=1, truncation="left", padding_side=side, return_plan=True)[-1]
        plan = host(plan_t)
        assert same(plan, F.padded_plan(offs, L, bos_id=1, truncation="left", padding_side=side))
        for vals, fill in value_arrays(len(ids), rng):
            got = host(hutoken_amd.gather_rows(plan_t, L, dev(vals), fill=fill, check=True))
            assert same(got, F.gather(plan, L, vals, fill=fill)), (L, side, vals.dtype, vals.shape)
        # two sides of two arrays, and of one array (values_b=None)
        half = len(lens) // 2
        oa, ob = offs[:half + 1], offs[half:2 * half + 1]
        d_oa, d_ob = dev(oa), dev(ob)
        plan_t = hutoken_amd.collate_pairs(d_ids, d_oa, d_ids, d_ob, L, padding_side=side, return_plan=True,
                                           **(TPL if L > 5 else {}))[-1]
        plan = host(plan_t)
        assert same(plan, F.pairs_plan(oa, ob, L, padding_side=side, **(TPL if L > 5 else {})))
        for (va, fill), (vb, _f) in zip(value_arrays(len(ids), rng), value_arrays(len(ids) + 3, rng)):
            got = host(hutoken_amd.gather_rows(plan_t, L, dev(va), dev(vb), fill=fill, check=True))
            assert same(got, F.gather(plan, L, va, vb, fill=fill)), (L, side, va.dtype, va.shape)
            got = host(hutoken_amd.gather_rows(plan_t, L, dev(va), fill=fill, check=True))
            assert same(got, F.gather(plan, L, va, fill=fill)), (L, side, va.dtype, va.shape)


def test_gather_without_rows_or_documents():
    import torch
    import hutoken_amd
    empty = hutoken_amd.collate_padded(dev(np.zeros(0, np.int32)), dev(np.zeros(1, np.int64)), 8, return_plan=True)[-1]
    out = hutoken_amd.gather_rows(empty, 8, torch.zeros((0, 2), dtype=torch.int32, device="cuda:0"), check=True)
    assert out.shape == (0, 8, 2) and out.dtype == torch.int32
    out = hutoken_amd.gather_rows(empty, 8, torch.zeros(0, dtype=torch.int64, device="cuda:0"), fill=3, check=True)
    assert out.shape == (0, 8) and out.dtype == torch.int64
    # documents without ids: rows of fill
    plan = hutoken_amd.collate_padded(dev(np.zeros(0, np.int32)), dev(np.zeros(4, np.int64)), 8, eos_id=2, return_plan=True)[-1]
    out = hutoken_amd.gather_rows(plan, 8, torch.zeros(0, dtype=torch.int32, device="cuda:0"), fill=-1, check=True)
    assert out.shape == (3, 8) and bool((out == -1).all())


def raw_gather(plan, L, va, vb, rec, fill_bytes, out):
    """hutk_rows_gather_device on tensors as they are (views included) -> the error word"""
    import torch
    from hutoken_amd import _capi
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    _capi.rows_gather_device(plan.data_ptr(), plan.shape[0], L, va.data_ptr(), va.shape[0], vb.data_ptr(), vb.shape[0], rec,
                             fill_bytes, out.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return int(err.item())


@pytest.mark.parametrize("L", [8, 6])
def test_gather_on_views_off_the_16_byte_boundary(L):
    """Values and output that begin 4 bytes (int32) or 8 bytes (int64) behind a 16-byte boundary: the path that moves a
    record dword by dword, with the same result."""
    import struct
    import torch
    import hutoken_amd
    rng = np.random.default_rng(7)
    ids, offs = ragged(list(rng.integers(0, 2 * L, size=300)), rng)
    plan_t = hutoken_amd.collate_padded(dev(ids), dev(offs), L, eos_id=2, return_plan=True)[-1]
    plan = host(plan_t)
    n_rows = len(plan)
    for vals, fill, code in ((rng.integers(-2**31, 2**31, size=len(ids)).astype(np.int32), (-1,), "i"),
                             (rng.integers(-2**31, 2**31, size=(len(ids), 2)).astype(np.int32), (0, -7), "ii"),
                             (rng.integers(-2**62, 2**62, size=(len(ids), 2)).astype(np.int64), (5, -1), "qq")):
        per = vals.shape[1] if vals.ndim == 2 else 1
        want = F.gather(plan, L, vals, fill=fill if per == 2 else fill[0])
        tdt = torch.int32 if vals.dtype == np.int32 else torch.int64
        rec = vals.dtype.itemsize * per
        for off_v, off_o in ((1, 0), (0, 1), (1, 1)):  # elements the view begins behind its allocation
            store = torch.zeros(vals.size + 8, dtype=tdt, device="cuda:0")
            d_vals = store[off_v:off_v + vals.size].view(vals.shape)
            d_vals.copy_(dev(vals))
            big = torch.full((want.size + 8,), 77, dtype=tdt, device="cuda:0")
            out = big[off_o:off_o + want.size]
            assert d_vals.data_ptr() % 16 == off_v * vals.dtype.itemsize and out.data_ptr() % 16 == off_o * vals.dtype.itemsize
            assert raw_gather(plan_t, L, d_vals, d_vals, rec, struct.pack("<" + code, *fill), out) == 0
            assert same(host(out).reshape(want.shape), want), (L, vals.dtype, vals.shape, off_v, off_o)
            rest = host(big)
            assert (rest[:off_o] == 77).all() and (rest[off_o + want.size:] == 77).all()


def hostile_reference(plan, L, va, vb, fill):
    """What the gather makes of any plan: the sides clipped to the row, A in front of B, fill for a record outside its
    array -> (rows, whether something was wrong)"""
    out = np.full((len(plan), L), fill, dtype=va.dtype)
    wrong = False
    for r, (_i, _s, sa, ka, ca, sb, kb, cb) in enumerate(plan.tolist()):
        claimed = np.zeros(L, dtype=bool)
        for src, k, col, vals in ((sa, ka, ca, va), (sb, kb, cb, vb)):
            if k < 0:
                wrong = True
            if k <= 0:
                continue
            if col < 0 or col + k > L:
                wrong = True
            for c in range(max(col, 0), min(col + k, L)):
                if claimed[c]:
                    wrong = True
                    continue
                claimed[c] = True
                j = src + (c - col)
                if 0 <= j < len(vals):
                    out[r, c] = vals[j]
                else:
                    wrong = True
    return out, wrong


def test_gather_of_a_hostile_plan_stays_inside_its_buffers():
    """A plan is a caller's tensor.  Whatever it holds the gather reads no record outside the values and writes nothing
    outside the rows: an error path with a defined result, HUTK_E_ARG and a guard band left as it was."""
    import struct
    import torch
    import hutoken_amd
    rng = np.random.default_rng(9)
    n_a, n_b = 40, 25
    va, vb = rng.integers(1, 1000, size=n_a).astype(np.int32), rng.integers(1000, 2000, size=n_b).astype(np.int32)
    d_va, d_vb = dev(va), dev(vb)
    big = 2**62
    for L in (8, 7, 4100):
        whole = min(L, n_a)
        sound = [[0, 0, 3, 4, 1, 2, 2, 5], [1, 0, 0, 0, 0, 0, 0, 0], [2, 0, n_a - whole, whole, 0, 0, 0, whole]]
        defects = {"src_a behind the values": [0, 0, n_a - 2, 4, 0, 0, 0, 4],
                   "src_a negative": [0, 0, -3, 4, 0, 0, 0, 4],
                   "src_b far away": [0, 0, 0, 2, 0, big, 3, 3],
                   "src_a at the lowest value": [0, 0, -2**63, 2, 0, 0, 0, 2],
                   "ka negative": [0, 0, 0, -5, 0, 1, 2, 3],
                   "kb negative": [0, 0, 0, 2, 0, 1, -big, 3],
                   "col_a beyond the row": [0, 0, 0, 3, L + 3, 0, 0, L + 6],
                   "col_a at the row's end": [0, 0, 0, 1, L, 0, 0, L + 1],
                   "col_b negative": [0, 0, 0, 2, 0, 4, 3, -2],
                   "col_a far away": [0, 0, 0, 3, big, 0, 3, -big],
                   "ka leaves the row": [0, 0, 0, L + 1, 0, 0, 0, L + 1],
                   "ka huge": [0, 0, 0, 2**63 - 1, 2, 0, 2**63 - 1, 2**63 - 1],
                   "kb leaves the row": [0, 0, 0, 2, 0, 0, L, 2],
                   "sides overlap": [0, 0, 0, 4, 1, 5, 3, 3]}
        fill = -4
        for name, rows in [("sound", sound)] + [(k, [v]) for k, v in defects.items()] + [("all", sound + list(defects.values()))]:
            plan = np.array(rows, dtype=np.int64)
            want, wrong = hostile_reference(plan, L, va, vb, fill)
            assert wrong == (name != "sound"), name
            guard = 64
            store = torch.full((guard + want.size + guard,), 77, dtype=torch.int32, device="cuda:0")
            out = store[guard:guard + want.size]
            assert out.data_ptr() % 16 == 0
            rc = raw_gather(dev(plan), L, d_va, d_vb, 4, struct.pack("<i", fill), out)
            assert rc == (E_ARG if wrong else 0), (L, name, rc)
            got = host(store)
            assert (got[:guard] == 77).all() and (got[guard + want.size:] == 77).all(), (L, name)
            assert same(got[guard:guard + want.size].reshape(want.shape), want), (L, name)
            if wrong:
                with pytest.raises(ValueError, match="row_plan"):
                    hutoken_amd.gather_rows(dev(plan), L, d_va, d_vb, fill=fill, check=True)
            else:
                assert same(host(hutoken_amd.gather_rows(dev(plan), L, d_va, d_vb, fill=fill, check=True)), want)


# ---- texts: ids, spans and word starts, computed once -----------------------------------------------------------------
def init(preset):
    import hutoken_amd
    from hutoken_amd import data
    vp, sp, _kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, is_byte_encoder=True, pretokenizer=preset)
    return hutoken_amd


def pack(texts):
    raw = [t.encode("utf-8") for t in texts]
    offs = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in raw], out=offs[1:])
    return np.frombuffer(b"".join(raw), dtype=np.uint8).copy(), offs, raw


@functools.lru_cache(maxsize=None)
def _token_text():
    from hutoken_amd import data
    from oracle import oracle
    oracle.build()
    vp, sp, kw = data.vocab_files("VG")
    return S.TokenText(oracle.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]))


@functools.lru_cache(maxsize=None)
def reference(preset, texts):
    """The GPU's ids of `texts` under the preset with what the restatement says of them: byte and character spans, word
    ids.  Computed once per (preset, texts) and shared; nobody changes it."""
    hutoken = init(preset)
    data, offs, raw = pack(list(texts))
    docs = hutoken.batch_encode(list(texts))
    oo = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=oo[1:])
    ids = np.array([t for d in docs for t in d], dtype=np.int32)
    assert not (ids == -1).any()
    tt = _token_text()
    spans_b, st = S.batch(tt, data, offs, ids, oo, True, "byte", np.int32)
    spans_c, _st = S.batch(tt, data, offs, ids, oo, True, "char", np.int32)
    assert not st.any()
    words = np.zeros(len(ids), dtype=np.int32)
    for i, doc in enumerate(raw):
        w, mismatch = F.word_ids(doc, spans_b[oo[i]:oo[i + 1]].tolist(), SR.word_starts(doc, preset))
        assert not mismatch
        words[oo[i]:oo[i + 1]] = w
    return dict(data=data, offs=offs, raw=raw, ids=ids, oo=oo, byte=spans_b, char=spans_c, words=words)


def on_device(ref):
    return dev(ref["data"]), dev(ref["offs"]), dev(ref["ids"]), dev(ref["oo"])


# ---- word ids ---------------------------------------------------------------------------------------------------------
def word_id_texts():
    from hutoken_amd import _capi
    tile, chunk = _capi.word_ids_tile(), _capi.presplit_chunk_bytes()
    long_one = FC.long_text(max(chunk + 500, 5 * tile))  # crosses a chunk of the split and, in ids, a tile of the rank kernel
    return tuple(FC.short_texts(100) + ["", long_one, ""] + FC.NER_TEXTS + ["", ""])


@pytest.mark.parametrize("preset", PRESETS)
def test_word_ids(preset):
    from hutoken_amd import _capi
    texts = word_id_texts()
    ref = reference(preset, texts)
    hutoken = init(preset)
    lens = np.diff(ref["oo"])
    assert lens.max() > _capi.word_ids_tile() and (lens == 0).any() and (np.diff(ref["offs"])[:100] < 32).all()
    assert np.diff(ref["offs"]).max() > _capi.presplit_chunk_bytes()
    inside = [ref["data"][ref["offs"][i] + a] & 0xC0 == 0x80 for i in range(len(texts))
              for a, b in ref["byte"][ref["oo"][i]:ref["oo"][i + 1]].tolist() if b > a]
    assert any(inside)  # some token begins inside a character: the byte-level tokens split it
    d_bytes, d_offs, d_ids, d_oo = on_device(ref)
    for kw in ({}, {"n_ids": len(ref["ids"])}, {"preset": preset, "check": False}):
        got = hutoken.token_word_ids_device(d_bytes, d_offs, d_ids, d_oo, **kw)
        assert got.dtype.is_signed and same(host(got), ref["words"]), kw
    # a token that is part of a character belongs to the character's word
    doc = texts.index("日本語のテキスト 123")
    a, b = ref["oo"][doc], ref["oo"][doc + 1]
    assert b - a > 5 and (np.diff(ref["words"][a:b]) >= 0).all() and ref["words"][a] == 0


def test_word_ids_of_ids_made_under_another_split():
    """Ids encoded under gpt2 and asked under cl100k: the documents on which the splits differ so that a token holds a
    word start strictly inside it are reported, each of them and no other; the other documents' word ids are exact."""
    import torch
    from hutoken_amd import _capi
    texts = ("hello world", "we'll see 12345", "", "a b c", "12345678 and 87654321", "no numbers here")
    ref = reference("gpt2", texts)
    want, flagged = np.zeros(len(ref["ids"]), dtype=np.int32), []
    for i, doc in enumerate(ref["raw"]):
        a, b = ref["oo"][i], ref["oo"][i + 1]
        w, mismatch = F.word_ids(doc, ref["byte"][a:b].tolist(), SR.word_starts(doc, "cl100k"))
        want[a:b] = w
        flagged.append(mismatch)
    assert flagged == [False, True, False, False, True, False]
    hutoken = init("gpt2")
    d_bytes, d_offs, d_ids, d_oo = on_device(ref)
    with pytest.raises(ValueError, match="document 1: .*cl100k"):
        hutoken.token_word_ids_device(d_bytes, d_offs, d_ids, d_oo, preset="cl100k")
    got = host(hutoken.token_word_ids_device(d_bytes, d_offs, d_ids, d_oo, preset="cl100k", check=False))
    assert same(got, want)
    assert same(host(hutoken.token_word_ids_device(d_bytes, d_offs, d_ids, d_oo)), ref["words"])  # under its own split
    # the status of every document, through the C ABI
    n_docs, n_bytes, n_ids = len(texts), len(ref["data"]), len(ref["ids"])
    bits = hutoken.pretokenize_packed_device(d_bytes, d_offs, "cl100k", return_bits=True)
    before = torch.zeros(n_bytes // 32 + 2, dtype=torch.int64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    hutoken._pretokenizer(d_bytes.device).starts_device(bits.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, before.data_ptr(), 0, 0, stream)
    for width, dt in ((4, np.int32), (8, np.int64)):
        spans = dev(ref["byte"].astype(dt))
        words = torch.full((n_ids,), -5, dtype=torch.int32, device="cuda:0")
        status = torch.full((n_docs,), -5, dtype=torch.int32, device="cuda:0")
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        _capi.token_word_ids_device(bits.data_ptr(), before.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, spans.data_ptr(), width,
                                    d_oo.data_ptr(), n_ids, words.data_ptr(), status.data_ptr(), err.data_ptr(), stream)
        assert int(err.item()) == E_UNSUPPORTED and same(host(words), want)
        assert host(status).tolist() == [S.MISMATCH if f else 0 for f in flagged]
    # id offsets that do not describe the ids: HUTK_E_ARG and nothing is written
    for bad in (ref["oo"] + 1, np.concatenate([ref["oo"][:-1], [n_ids + 1]])):
        words = torch.full((n_ids,), -5, dtype=torch.int32, device="cuda:0")
        d_bad = dev(bad.astype(np.int64))
        _capi.token_word_ids_device(bits.data_ptr(), before.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, spans.data_ptr(), 8,
                                    d_bad.data_ptr(), n_ids, words.data_ptr(), 0, err.data_ptr(), stream)
        assert int(err.item()) == E_ARG and bool((words == -5).all())


# ---- answers ----------------------------------------------------------------------------------------------------------
def qa_rows(preset, L=32, stride=8, strategy="only_second"):
    """The QA pairs as windows with their plan -> (plan on the device, its host copy, reference of the one encode call)"""
    texts = tuple(FC.QUESTIONS + FC.CONTEXTS)
    ref = reference(preset, texts)
    hutoken = init(preset)
    n = len(FC.QUESTIONS)
    res = hutoken.batch_encode_pair_windows(FC.QUESTIONS, FC.CONTEXTS, L, stride, truncation=strategy, return_plan=True,
                                            pad_id=-9, **TPL)
    plan = host(res[-1])
    assert same(plan, F.pair_windows_plan(ref["oo"][:n + 1], ref["oo"][n:], L, stride, strategy, **TPL))
    return res[-1], plan, ref


def check_answers(hutoken, d_plan, plan, spans, ans, side="b", dtype=np.int32):
    got = host(hutoken.answer_positions(d_plan, dev(spans.astype(dtype)), dev(np.asarray(ans, dtype=dtype)), side=side, check=True))
    want = F.answers(plan, side, spans, ans)
    assert got.dtype == np.int32 and same(got, want), (got[:8], want[:8])
    return got


@pytest.mark.parametrize("preset", PRESETS)
def test_answer_positions(preset):
    import hutoken_amd as hutoken
    d_plan, plan, ref = qa_rows(preset)
    n = len(FC.QUESTIONS)
    spans, ob = ref["char"], ref["oo"][n:]
    none = np.full((n, 2), -1, dtype=np.int64)
    assert (check_answers(hutoken, d_plan, plan, spans, none) == -1).all()
    rows_of = lambda i: np.nonzero(plan[:, 0] == i)[0]  # noqa: E731
    item = 2  # twenty sentences: several windows
    rows = rows_of(item)
    assert len(rows) >= 3
    first, last = int(ob[item]), int(ob[item + 1]) - 1
    # the first token and the last token of the context
    ans = none.copy()
    ans[item] = spans[first]
    got = check_answers(hutoken, d_plan, plan, spans, ans)
    assert got[rows[0]].tolist() == [plan[rows[0], 7]] * 2 and (got[rows[2:]] == -1).all()
    ans[item] = spans[last]
    got = check_answers(hutoken, d_plan, plan, spans, ans, dtype=np.int64)
    end_col = plan[rows[-1], 7] + plan[rows[-1], 6] - 1
    assert got[rows[-1]].tolist() == [end_col] * 2 and (got[rows_of(0)] == -1).all()
    # inside the stride's overlap: found in two rows, at columns 24 - 8 = 16 apart less what the window moved by
    r0, r1 = rows[0], rows[1]
    j = int(plan[r1, 5])  # the first token of the second window: one of the last 8 of the first
    assert plan[r0, 5] < j < plan[r0, 5] + plan[r0, 6]
    ans[item] = (spans[j][0], spans[j + 1][1])
    got = check_answers(hutoken, d_plan, plan, spans, ans)
    in_r0 = int(plan[r0, 7] + j - plan[r0, 5])
    assert got[r1].tolist() == [plan[r1, 7], plan[r1, 7] + 1] and got[r0].tolist() == [in_r0, in_r0 + 1]
    assert (got[rows[2:]] == -1).all()
    # across the first window's edge: not in the row that holds only its beginning
    j = int(plan[r0, 5] + plan[r0, 6]) - 1  # the first window's last token
    ans[item] = (spans[j][0], spans[j + 1][1])
    got = check_answers(hutoken, d_plan, plan, spans, ans)
    assert got[r0].tolist() == [-1, -1] and got[r1][0] >= 0 and got[r1][1] == got[r1][0] + 1
    # every item at once: an answer in the middle of every context that has one; the empty context has none
    for i in range(n):
        a, b = int(ob[i]), int(ob[i + 1])
        ans[i] = (spans[(a + b) // 2][0], spans[min((a + b) // 2 + 2, b - 1)][1]) if b > a else (0, 1)
    got = check_answers(hutoken, d_plan, plan, spans, ans)
    assert FC.CONTEXTS[3] == "" and (got[rows_of(3)] == -1).all()
    assert all((got[rows_of(i)] >= 0).any() for i in (0, 2, 4))  # (their questions leave room for three tokens and more)
    # characters in the middle of a token: the token that holds the character
    lo, hi = (int(x) for x in spans[first + 1])
    if hi - lo >= 3:
        ans = none.copy()
        ans[item] = (lo + 1, hi - 1)
        assert check_answers(hutoken, d_plan, plan, spans, ans)[rows[0]].tolist() == [plan[rows[0], 7] + 1] * 2


def test_answer_that_begins_inside_a_character_the_tokens_split():
    import hutoken_amd as hutoken
    d_plan, plan, ref = qa_rows("gpt2")
    n = len(FC.QUESTIONS)
    spans, ob = ref["byte"], ref["oo"][n:]
    item = 6  # the context that begins with kanji: three bytes a character, some of them several tokens
    assert FC.CONTEXTS[item].startswith("日本語")
    doc = ref["raw"][n + item]
    toks = spans[ob[item]:ob[item + 1]]
    inner = [k for k, (a, b) in enumerate(toks.tolist()) if b > a and doc[a] & 0xC0 == 0x80]  # begins inside a character
    assert inner and inner[0] < 12, toks[:10]
    k = inner[0]
    ans = np.full((n, 2), -1, dtype=np.int64)
    ans[item] = (toks[k][0], toks[k][1])
    got = check_answers(hutoken, d_plan, plan, spans, ans)
    row = np.nonzero(plan[:, 0] == item)[0][0]
    assert got[row].tolist() == [plan[row, 7] + k] * 2
    ans[item] = (toks[k][0] - 1, toks[k][1])  # one byte earlier: the token before it holds the start
    assert check_answers(hutoken, d_plan, plan, spans, ans)[row].tolist() == [plan[row, 7] + k - 1, plan[row, 7] + k]


def test_answers_on_the_first_side():
    import hutoken_amd as hutoken
    d_plan, plan, ref = qa_rows("cl100k", L=24, stride=3, strategy="only_first")
    n = len(FC.QUESTIONS)
    spans, oa = ref["char"], ref["oo"][:n + 1]
    ans = np.full((n, 2), -1, dtype=np.int64)
    for i in range(n):
        a, b = int(oa[i]), int(oa[i + 1])
        if b > a:
            ans[i] = (spans[a][0], spans[b - 1][1])  # the whole question
    got = check_answers(hutoken, d_plan, plan, spans, ans, side="a")
    whole = plan[:, 3] == np.diff(oa)[plan[:, 0]]
    assert ((got[:, 0] >= 0) == (whole & (plan[:, 3] > 0))).all()
    # a plan that points outside the spans or the answers: reported, nothing read there
    bad = plan.copy()
    bad[0, 0] = n
    bad[1, 2] = len(spans) - 1
    bad[1, 3] = 5
    with pytest.raises(ValueError, match="row_plan"):
        hutoken.answer_positions(dev(bad), dev(spans), dev(ans.astype(np.int32)), side="a", check=True)
    res = host(hutoken.answer_positions(dev(bad), dev(spans), dev(ans.astype(np.int32)), side="a"))
    assert res[0].tolist() == [-1, -1] and res[1].tolist() == [-1, -1] and same(res[2:], got[2:])


# ---- end to end -------------------------------------------------------------------------------------------------------
def check_rectangles(texts_of_side, ref, plan, L, input_ids, mapping, word_ids):
    """offset_mapping and word_ids against the restatement, and the texts sliced by the mapping against the decoded
    tokens.  texts_of_side: (texts of A, texts of B or None) -- the str a row's item refers to on either side."""
    assert mapping.dtype == np.int32 and word_ids.dtype == np.int32
    assert same(mapping, F.gather(plan, L, ref["char"], fill=0))
    assert same(word_ids, F.gather(plan, L, ref["words"], fill=-1))
    tt = _token_text()
    sliced = 0
    for r, (item, _s, sa, ka, ca, sb, kb, cb) in enumerate(plan.tolist()):
        for src, k, col, texts in ((sa, ka, ca, texts_of_side[0]), (sb, kb, cb, texts_of_side[1])):
            for q in range(k):
                a, b = mapping[r, col + q].tolist()
                try:
                    piece = tt.rest(int(input_ids[r, col + q])).decode("utf-8")
                except UnicodeDecodeError:
                    continue  # (a token that is part of a character has no text of its own)
                assert texts[item][a:b] == piece, (r, q, texts[item][a:b], piece)
                sliced += 1
        on_token = np.zeros(L, dtype=bool)
        on_token[ca:ca + ka] = True
        on_token[cb:cb + kb] = True
        assert (word_ids[r][~on_token] == -1).all() and (word_ids[r][on_token] >= 0).all() and not mapping[r][~on_token].any()
    return sliced


@pytest.mark.parametrize("preset", PRESETS)
def test_end_to_end_pair_windows(preset):
    texts = tuple(FC.QUESTIONS + FC.CONTEXTS)
    ref = reference(preset, texts)
    hutoken = init(preset)
    n, L, stride = len(FC.QUESTIONS), 32, 8
    res = hutoken.batch_encode_pair_windows(FC.QUESTIONS, FC.CONTEXTS, L, stride, pad_id=-9, return_offsets_mapping=True,
                                            return_word_ids=True, **TPL)
    assert len(res) == 7
    plan = F.pair_windows_plan(ref["oo"][:n + 1], ref["oo"][n:], L, stride, **TPL)
    got = [host(x) for x in res]
    assert same(got[0], F.rebuild(plan, L, ref["ids"], pad_id=-9, **TPL)) and same(got[4], plan[:, :2])
    assert check_rectangles((FC.QUESTIONS, FC.CONTEXTS), ref, plan, L, got[0], got[5], got[6]) > 500
    # the B side's word ids count from 0 again: each side is its own document
    first_b = got[6][np.arange(len(plan)), plan[:, 7]][(plan[:, 6] > 0) & (plan[:, 1] == 0)]
    assert len(first_b) and not first_b.any()
    # with the plan asked for, it comes before the features; bytes instead of characters
    res = hutoken.batch_encode_pair_windows(FC.QUESTIONS, FC.CONTEXTS, L, stride, pad_id=-9, return_offsets_mapping=True,
                                            offsets_unit="byte", return_plan=True, **TPL)
    assert len(res) == 7 and same(host(res[5]), plan) and same(host(res[6]), F.gather(plan, L, ref["byte"], fill=0))
    res = hutoken.batch_encode_pair_windows(FC.QUESTIONS, FC.CONTEXTS, L, stride, pad_id=-9, return_word_ids=True, **TPL)
    assert len(res) == 6 and same(host(res[5]), got[6])


@pytest.mark.parametrize("preset", PRESETS)
def test_end_to_end_padded_windows_and_pairs(preset):
    texts = tuple(FC.NER_TEXTS + FC.CONTEXTS)
    ref = reference(preset, texts)
    hutoken = init(preset)
    texts = list(texts)
    for L, side, tr in ((16, "right", "right"), (12, "left", "left")):
        res = [host(x) for x in hutoken.batch_encode_padded(texts, L, bos_id=1, pad_id=-9, padding_side=side, truncation=tr,
                                                            return_offsets_mapping=True, return_word_ids=True)]
        plan = F.padded_plan(ref["oo"], L, bos_id=1, truncation=tr, padding_side=side)
        assert len(res) == 5 and same(res[0], F.rebuild(plan, L, ref["ids"], bos_id=1, pad_id=-9))
        assert check_rectangles((texts, None), ref, plan, L, res[0], res[3], res[4]) > 50
    res = [host(x) for x in hutoken.batch_encode_padded(texts, return_word_ids=True)]  # padded to the longest
    assert len(res) == 4 and same(res[3], F.gather(F.padded_plan(ref["oo"], res[0].shape[1]), res[0].shape[1], ref["words"], fill=-1))
    for L, stride, side in ((16, 4, "right"), (9, 0, "left")):
        res = [host(x) for x in hutoken.batch_encode_windows(texts, L, stride, eos_id=2, pad_id=-9, padding_side=side,
                                                             return_offsets_mapping=True, return_word_ids=True)]
        plan = F.windows_plan(ref["oo"], L, stride, eos_id=2, padding_side=side)
        assert len(res) == 6 and same(res[0], F.rebuild(plan, L, ref["ids"], eos_id=2, pad_id=-9)) and same(res[3], plan[:, :2])
        assert check_rectangles((texts, None), ref, plan, L, res[0], res[4], res[5]) > 100
    n = len(FC.NER_TEXTS)
    ta, tb = texts[:8], texts[n:n + 8]
    pair_ref = reference(preset, tuple(ta + tb))
    for L, strategy, side in ((24, "longest_first", "right"), (20, "only_second", "left"), (20, "only_first", "right")):
        res = [host(x) for x in hutoken.batch_encode_pairs(ta, tb, L, truncation=strategy, padding_side=side, pad_id=-9,
                                                           return_offsets_mapping=True, return_word_ids=True, **TPL)]
        plan = F.pairs_plan(pair_ref["oo"][:9], pair_ref["oo"][8:], L, strategy, padding_side=side, **TPL)
        assert len(res) == 6 and same(res[0], F.rebuild(plan, L, pair_ref["ids"], pad_id=-9, **TPL))
        assert check_rectangles((ta, tb), pair_ref, plan, L, res[0], res[4], res[5]) > 50
    hutoken.set_pretokenizer(None)  # the built-in splitter: word ids are refused before anything is encoded
    with pytest.raises(ValueError, match="split preset"):
        hutoken.batch_encode_padded(texts, 16, return_word_ids=True)
    res = hutoken.batch_encode_padded(texts[:3], 16, return_offsets_mapping=True)  # the mapping needs no preset
    assert len(res) == 4 and res[3].shape == (3, 16, 2)


# ---- streams ----------------------------------------------------------------------------------------------------------
def features_run(hutoken, ref):
    n = len(FC.QUESTIONS)
    res = hutoken.batch_encode_pair_windows(FC.QUESTIONS, FC.CONTEXTS, 32, 8, pad_id=-9, return_plan=True,
                                            return_offsets_mapping=True, return_word_ids=True, **TPL)
    ans = np.array([(0, 5)] * n, dtype=np.int32)
    pos = hutoken.answer_positions(res[5], dev(ref["char"]), dev(ans))
    rect = hutoken.gather_rows(res[5], 32, dev(ref["byte"].astype(np.int64)), fill=(-1, -1))
    return res + (pos, rect)


def test_on_the_default_and_on_a_non_default_stream():
    import torch
    ref = reference("gpt2", tuple(FC.QUESTIONS + FC.CONTEXTS))
    hutoken = init("gpt2")
    assert torch.cuda.current_stream().cuda_stream == 0
    on_default = [host(x) for x in features_run(hutoken, ref)]
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        on_side = features_run(hutoken, ref)
        torch.cuda.synchronize()
    assert len(on_default) == 10 and all(same(a, host(b)) for a, b in zip(on_default, on_side))
    n = len(FC.QUESTIONS)
    plan = F.pair_windows_plan(ref["oo"][:n + 1], ref["oo"][n:], 32, 8, **TPL)
    assert same(on_default[5], plan) and same(on_default[6], F.gather(plan, 32, ref["char"], fill=0))
    assert same(on_default[8], F.answers(plan, "b", ref["char"], [(0, 5)] * n))
    assert same(on_default[9], F.gather(plan, 32, ref["byte"].astype(np.int64), fill=(-1, -1)))
