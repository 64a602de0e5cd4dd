"""Span corruption on the GPU (csrc/hutk_collate.hip: k_rows_span_corrupt) against the numpy restatement of
tests/span_ref.py, every comparison exact and over every element of every output, for int32 and int64 rows.

The rows and their plans are the library's own (collate_* with return_plan=True) over random ids; the start threshold
and the length table come from the same arithmetic on both sides (span_ref.thresholds restates corrupt_spans').  Needs a
real MI355X."""
import numpy as np
import pytest

import features_cases as FC
import span_ref as S

pytestmark = pytest.mark.gpu

E_ARG = 4
FIRST = 60000  # the first sentinel: the random ids lie below 50000
WIDTHS = ("int32", "int64")
SIDES = {"a": 1, "b": 2, "both": 3}
NAMES = ("input_ids", "attention_mask", "labels", "input_lengths", "target_lengths", "decoder_input_ids")
ALWAYS_32 = [0.0] * 31 + [1.0]  # every span is drawn 32 columns long


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
    return rng.integers(100, 50000, size=int(offs[-1])).astype(np.int32), offs


def padded(lens, L, dtype, rng, **kw):
    import hutoken_amd
    ids, offs = ragged(lens, rng)
    return hutoken_amd.collate_padded(dev(ids), dev(offs), L, dtype=dtype, return_plan=True, check=True, **kw)


def reference(ids, mask, plan, *, seed, density=0.15, probs=None, mean=3.0, max_span=10, first=FIRST, step=-1, n_sent=100, eos=7,
              start=None, L_tgt=None, pad=0, ignore=-100, sides="both", first_row=0):
    return S.span_corrupt_ref(ids, mask, plan, seed=seed, sentinel_first=first, sentinel_step=step, n_sentinels=n_sent, target_eos_id=eos,
                              decoder_start_id=start, pad_id=pad, ignore_index=ignore, sides=SIDES[sides], max_target_len=L_tgt,
                              first_row=first_row, **S.thresholds(density, mean, max_span, probs))


def check(ids_t, mask_t, plan_t, *, seed, density=0.15, probs=None, mean=3.0, max_span=10, first=FIRST, step=-1, n_sent=100, eos=7,
          start=None, L_tgt=None, pad=0, ignore=-100, sides="both"):
    """corrupt_spans against the restatement -> the outputs on the host, decoder_input_ids or None the last"""
    import hutoken_amd
    res = hutoken_amd.corrupt_spans(ids_t, mask_t, plan_t, sentinel_first=first, seed=seed, noise_density=density, mean_span_length=mean,
                                    max_span_length=max_span, span_length_probs=probs, n_sentinels=n_sent, sentinel_step=step,
                                    target_eos_id=eos, decoder_start_id=start, max_target_length=L_tgt, pad_id=pad, ignore_index=ignore,
                                    sides=sides, check=True)
    assert len(res) == (5 if start is None else 6)
    want = reference(host(ids_t), host(mask_t), host(plan_t), seed=seed, density=density, probs=probs, mean=mean, max_span=max_span,
                     first=first, step=step, n_sent=n_sent, eos=eos, start=start, L_tgt=L_tgt, pad=pad, ignore=ignore, sides=sides)
    assert not want[6]
    got = [host(x) for x in res]
    for name, g, w in zip(NAMES, got, want):
        assert same(g, w), (name, tuple(ids_t.shape), seed, sides)
    assert res[0].dtype == ids_t.dtype and res[2].dtype == ids_t.dtype
    return got + [None] * (6 - len(got))


# ---- chunk edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [1, 3, 4, 5, 255, 256, 257, 260, 511, 512, 513, 1027])
def test_row_lengths(L, dtype):
    """One column; the path of single loads (3, 5, 255, 257, 511, 513, 1027) and that of four at once; one chunk of 256
    columns exactly, one column short of it and one column into the next; several chunks.  Either padding side, either
    truncation side, with and without bos and eos."""
    rng = np.random.default_rng(L)
    n = 12
    lens = [L + 5, 0, max(L - 3, 0), L] + list(rng.integers(0, 2 * L + 2, size=n - 4))
    for tpl in (dict(bos_id=1, eos_id=2), {}) if L >= 3 else ({},):
        for side, tr in (("right", "left"), ("left", "right")):
            ids_t, mask_t, lengths, plan_t = padded(lens, L, dtype, rng, padding_side=side, truncation=tr, pad_id=9, **tpl)
            assert ids_t.shape == (n, L) and int(lengths.max()) == L
            got = check(ids_t, mask_t, plan_t, seed=L, density=0.3, start=5, pad=9)
            if L >= 255:
                assert (got[4] > 20).any() and (got[3] < L).any()
            check(ids_t, mask_t, plan_t, seed=L + 1, density=0.6, mean=5.0, max_span=32, eos=None, L_tgt=L // 2 + 1, step=1)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_runs_across_the_chunk_edges(dtype):
    """Spans of 32 columns that start at one column in twenty: among the seeds 0 .. 63 the restatement finds one with a row
    that has a run over the columns 255 | 256 and another over 511 | 512, and one with a row whose run ends exactly with
    column 255 (one seed in a hundred does that to a given row: six full rows are looked at)."""
    rng = np.random.default_rng(2)
    L = 1027
    density = 1 - 0.95**32
    assert abs(S.thresholds(density, span_length_probs=ALWAYS_32)["start_below"] / 2**32 - 0.05) < 1e-9
    ids_t, mask_t, _lengths, plan_t = padded([L + 9, L, L, L, L + 1, L, 700], L, dtype, rng)
    mask, plan = host(mask_t), host(plan_t)
    across, ends = None, None
    for seed in range(64):
        for noise in S.noise_columns(mask[:6], plan[:6], seed=seed, **S.thresholds(density, span_length_probs=ALWAYS_32))[0]:
            runs = S.runs_of(noise)
            if across is None and noise[255] and noise[256] and noise[511] and noise[512] and not any(a <= 255 and b > 512 for a, b in runs):
                across = seed
            if ends is None and any(b == 256 for _a, b in runs):
                ends = seed
        if across is not None and ends is not None:
            break
    assert across is not None and ends is not None
    for seed in (across, ends):
        check(ids_t, mask_t, plan_t, seed=seed, density=density, probs=ALWAYS_32, start=5)


@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [8, 260])
def test_row_counts(L, dtype):
    """A workgroup holds four rows, one per wavefront: fewer, exactly four, a ragged last workgroup; rows of different
    lengths next to each other."""
    rng = np.random.default_rng(100 + L)
    for n in (1, 3, 4, 5, 9):
        ids_t, mask_t, _lengths, plan_t = padded([L] + list(rng.integers(0, L + 3, size=n - 1)), L, dtype, rng, eos_id=2, pad_id=9)
        check(ids_t, mask_t, plan_t, seed=n, density=0.4, start=5, pad=9)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_no_rows(dtype):
    import hutoken_amd
    res = hutoken_amd.collate_padded(dev(np.zeros(0, np.int32)), dev(np.zeros(1, np.int64)), 8, dtype=dtype, return_plan=True)
    got = hutoken_amd.corrupt_spans(res[0], res[1], res[3], sentinel_first=FIRST, seed=1, decoder_start_id=0, max_target_length=5, check=True)
    assert [tuple(x.shape) for x in got] == [(0, 8), (0, 8), (0, 5), (0,), (0,), (0, 5)] and got[2].dtype == res[0].dtype
    # documents without ids: rows of template and padding, nothing to corrupt
    res = hutoken_amd.collate_padded(dev(np.zeros(0, np.int32)), dev(np.zeros(4, np.int64)), 8, eos_id=2, pad_id=9, dtype=dtype, return_plan=True)
    got = check(res[0], res[1], res[3], seed=1, density=1.0, probs=[1.0], pad=9)
    assert same(got[0], host(res[0])) and got[2][:, 0].tolist() == [7] * 3 and got[4].tolist() == [1] * 3


# ---- extremes ---------------------------------------------------------------------------------------------------------
def rule_rows(dtype, L=512, n=10, seed=15, **kw):
    rng = np.random.default_rng(seed)
    return padded([L + 9, L - 2] + list(rng.integers(L // 2, L + 9, size=n - 2)), L, dtype, rng, bos_id=1, eos_id=2, pad_id=9, **kw)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_extremes(dtype):
    ids_t, mask_t, lengths, plan_t = rule_rows(dtype, padding_side="left")
    ids, mask, L = host(ids_t), host(mask_t), ids_t.shape[1]
    # nothing starts: the compacted input, and eos alone in the target
    got = check(ids_t, mask_t, plan_t, seed=1, density=0.0, pad=9)
    for r in range(len(ids)):
        n = int(mask[r].sum())
        assert got[0][r, :n].tolist() == ids[r][mask[r] != 0].tolist() and got[3][r] == n
    assert (got[2][:, 0] == 7).all() and (got[2][:, 1:] == -100).all() and (got[4] == 1).all()
    # every column starts a span of one: the side is one run, one sentinel
    got = check(ids_t, mask_t, plan_t, seed=1, density=1.0, probs=[1.0], pad=9)
    assert (got[0][:, :3] == np.array([1, FIRST, 2])).all() and (got[3] == 3).all() and same(got[4], host(lengths))  # sentinel + ids + eos
    # about 30 runs in a row, and 0, 1, 2 or all the sentinels; either step; short targets; no eos
    runs = [len(S.runs_of(x)) for x in S.noise_columns(mask, host(plan_t), seed=2, **S.thresholds(0.25))[0]]
    assert 10 < min(runs) and max(runs) < 70
    for n_sent in (0, 1, 2, 100):
        for step in (-1, 1):
            got = check(ids_t, mask_t, plan_t, seed=2, density=0.25, n_sent=n_sent, step=step, pad=9, start=5)
            used = np.unique(got[0][(got[0] >= FIRST - 99) & (got[0] <= FIRST + 99)])
            assert len(used) == min(n_sent, max(runs))
    for L_tgt in (1, 2, L):
        got = check(ids_t, mask_t, plan_t, seed=2, density=0.25, L_tgt=L_tgt, pad=9, start=5)
        assert (got[4] > 2).all() and got[2].shape == (len(ids), L_tgt)
    check(ids_t, mask_t, plan_t, seed=2, density=0.25, eos=None, pad=9, ignore=-1, L_tgt=3 * L)
    check(ids_t, mask_t, plan_t, seed=2, density=0.25, eos=None, start=5, first=3, step=1, n_sent=1000)


def test_wide_ids_sentinels_and_fills_go_through_whole():
    """int64 rows whose ids, sentinels, pad id and ignore index need more than 32 bits"""
    ids_t, mask_t, _lengths, plan_t = rule_rows("int64", L=40, n=8)
    got = check(ids_t + 2**40, mask_t, plan_t, seed=6, density=0.4, first=2**50, ignore=-2**50, start=5)
    assert (got[2][got[2] != -2**50] >= 7).all() and (got[2] >= 2**50 - 100).any() and (got[0][got[1] != 0] >= 2**40).all()


# ---- layouts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("n_sep", [1, 2])
def test_pairs(n_sep, dtype):
    """The three strategies, either side alone and both: the numbering of the runs goes on from A into B."""
    import hutoken_amd
    rng = np.random.default_rng(13 + n_sep)
    L = 48
    tpl = dict(bos_id=1, sep_ids=tuple(3 + i for i in range(n_sep)), eos_id=2, pad_id=9)
    R = L - 2 - n_sep
    lens = [(R // 2, R - R // 2), (R, R), (0, 2 * R), (2 * R, 0), (0, 0), (R + 3, 1), (1, R + 3), (R, 0), (0, R)]
    lens += [tuple(x) for x in rng.integers(0, L, size=(31, 2))]
    a, oa = ragged([x for x, _ in lens], rng, base=3)
    b, ob = ragged([y for _, y in lens], rng)
    for strategy, side in (("longest_first", "right"), ("only_first", "left"), ("only_second", "right")):
        res = hutoken_amd.collate_pairs(dev(a), dev(oa), dev(b), dev(ob), L, truncation=strategy, padding_side=side, dtype=dtype,
                                        return_plan=True, check=True, **tpl)
        ids_t, mask_t, plan_t = res[0], res[1], res[4]
        for sides in ("a", "b", "both"):
            got = check(ids_t, mask_t, plan_t, seed=31, density=0.4, sides=sides, pad=9, start=5)
        plan = host(plan_t)
        noise = S.noise_columns(host(mask_t), plan, seed=31, **S.thresholds(0.4))[0]
        in_both = 0
        for r, (_i, _s, _sa, ka, ca, _sb, kb, cb) in enumerate(plan.tolist()):
            row = got[0][r, :got[3][r]]
            used = row[row >= FIRST - 99].tolist()
            assert used == [FIRST - k for k in range(len(used))]  # counted through the row, both sides
            in_both += bool(noise[r, ca:ca + ka].any() and noise[r, cb:cb + kb].any())
        assert in_both > 5


@pytest.mark.parametrize("dtype", WIDTHS)
def test_windows_and_pair_windows(dtype):
    import hutoken_amd
    rng = np.random.default_rng(14)
    L, stride = 20, 3
    ids, offs = ragged([0, 14, 15, 100, 3, 41] + list(rng.integers(0, 60, size=20)), rng)
    for side in ("right", "left"):
        res = hutoken_amd.collate_windows(dev(ids), dev(offs), L, stride, bos_id=1, eos_id=2, pad_id=9, padding_side=side, dtype=dtype,
                                          return_plan=True, check=True)
        check(res[0], res[1], res[4], seed=21, density=0.4, pad=9, start=5)
    tpl = dict(bos_id=1, sep_ids=(3, 4), eos_id=2, pad_id=9)
    lens = [(3, 60), (0, 40), (5, 0), (16, 16), (30, 4)] + [(int(x), int(y)) for x, y in zip(rng.integers(0, 10, size=15), rng.integers(0, 60, size=15))]
    a, oa = ragged([x for x, _ in lens], rng)
    b, ob = ragged([y for _, y in lens], rng, base=2)
    for strategy, (x, ox, y, oy) in (("only_second", (a, oa, b, ob)), ("only_first", (b, ob, a, oa))):
        res = hutoken_amd.collate_pair_windows(dev(x), dev(ox), dev(y), dev(oy), L, stride, truncation=strategy, dtype=dtype, return_plan=True,
                                               check=True, **tpl)
        for sides in ("a", "b", "both"):
            check(res[0], res[1], res[5], seed=41, density=0.4, sides=sides, pad=9)


# ---- independence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
def test_a_row_depends_on_its_number_and_the_seed_alone(dtype):
    import torch
    import hutoken_amd
    ids_t, mask_t, _lengths, plan_t = rule_rows(dtype, L=260, n=9)
    kw = dict(sentinel_first=FIRST, noise_density=0.3, target_eos_id=7, decoder_start_id=5)
    whole = [host(x) for x in hutoken_amd.corrupt_spans(ids_t, mask_t, plan_t, seed=2**64 - 1, **kw)]
    again = [host(x) for x in hutoken_amd.corrupt_spans(ids_t, mask_t, plan_t, seed=2**64 - 1, **kw)]
    assert all(same(a, b) for a, b in zip(whole, again))
    for k in (1, 3, 5):  # the first k rows alone: a batch of another size
        part = hutoken_amd.corrupt_spans(ids_t[:k].contiguous(), mask_t[:k].contiguous(), plan_t[:k].contiguous(), seed=2**64 - 1, **kw)
        assert all(same(host(a), b[:k]) for a, b in zip(part, whole))
    other = [host(x) for x in hutoken_amd.corrupt_spans(ids_t, mask_t, plan_t, seed=2**63, **kw)]
    assert not same(other[0], whole[0]) and not same(other[2], whole[2])
    if dtype == "int64":  # the two widths give the same values
        narrow = hutoken_amd.corrupt_spans(ids_t.to(torch.int32), mask_t, plan_t, seed=2**64 - 1, **kw)
        assert all(same(host(a).astype(b.dtype), b) for a, b in zip(narrow, whole))


def guarded(n, dtype, guard=64):
    """n elements with a guard band on either side -> (the elements, the store)"""
    import torch
    store = torch.full((guard + n + guard,), 77, dtype=dtype, device="cuda:0")
    return store[guard:guard + n], store


def untouched(store, n, guard=64):
    rest = host(store)
    return bool((rest[:guard] == 77).all() and (rest[guard + n:] == 77).all())


def raw_span(plan, ids, mask, L, L_tgt, width, *, seed, th, first=FIRST, step=-1, n_sent=100, eos=7, start=5, pad=0, ignore=-100, sides=3,
             off_out=0, off_labels=0, dec_over=None):
    """hutk_rows_span_corrupt_device on tensors as they are (views included), every output inside guard bands
    -> (the error word, the six outputs on the host, whether every guard band is as it was).  dec_over: a tensor whose
    address is handed over as d_decoder_ids in place of the guarded one, which then must stay as it was."""
    import torch
    from hutoken_amd import _capi
    n = plan.shape[0]
    tdt = torch.int32 if width == 4 else torch.int64
    sizes = (n * L, n * L, n * L_tgt, n, n, n * L_tgt)
    dtypes = (tdt, torch.uint8, tdt, torch.int32, torch.int32, tdt)
    offs = (off_out, 0, off_labels, 0, 0, off_labels)
    pairs = [guarded(size + off, dt) for size, dt, off in zip(sizes, dtypes, offs)]
    views = [v[off:] for (v, _s), off in zip(pairs, offs)]
    err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    _capi.rows_span_corrupt_device(plan.data_ptr(), n, L, ids.data_ptr(), width, mask.data_ptr(), seed, th["start_below"], th["len_below"],
                                   first, step, n_sent, eos, start, pad, ignore, sides, L_tgt, views[0].data_ptr(), views[1].data_ptr(),
                                   views[2].data_ptr(), (views[5] if dec_over is None else dec_over).data_ptr(), views[3].data_ptr(), views[4].data_ptr(), err.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    shapes = ((n, L), (n, L), (n, L_tgt), (n,), (n,), (n, L_tgt))
    outs = [host(v).reshape(shape) for v, shape in zip(views, shapes)]
    clean = all(untouched(s, size + off) and bool((host(v)[:off] == 77).all()) for (v, s), size, off in zip(pairs, sizes, offs))
    return int(err.item()), outs, clean


def view_at(t, off):
    """a copy of t (flat) that begins `off` elements behind a 16-byte boundary"""
    import torch
    store = torch.full((t.numel() + 16,), 77, dtype=t.dtype, device="cuda:0")
    v = store[off:off + t.numel()]
    v.copy_(t.reshape(-1))
    assert v.data_ptr() % 16 == off * t.element_size() % 16
    return v


@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [8, 260])
def test_views_off_the_16_byte_boundary(L, dtype):
    """Inputs and outputs 4, 8 and 12 bytes behind a 16-byte boundary (int64: 8), the mask 1 .. 3 bytes behind a 4-byte one:
    the values of the aligned call, and nothing written around the outputs."""
    ids_t, mask_t, _lengths, plan_t = rule_rows(dtype, L=L, n=6)
    width = ids_t.element_size()
    th = S.thresholds(0.3)
    want = reference(host(ids_t), host(mask_t), host(plan_t), seed=5, density=0.3, start=5)
    steps = (1, 2, 3) if width == 4 else (1,)
    cases = [(0, 0, 0, 0)] + [(k, 0, 0, 0) for k in steps] + [(0, 0, k, 0) for k in steps] + [(0, 0, 0, k) for k in steps]
    cases += [(0, k, 0, 0) for k in (1, 2, 3)] + [(steps[-1], 3, steps[0], steps[-1])]
    for off_i, off_m, off_o, off_l in cases:
        rc, outs, clean = raw_span(plan_t, view_at(ids_t, off_i), view_at(mask_t, off_m), L, L, width, seed=5, th=th, off_out=off_o, off_labels=off_l)
        assert rc == 0 and clean, (off_i, off_m, off_o, off_l)
        for name, g, w in zip(NAMES, outs, want):
            assert same(g, w), (name, off_i, off_m, off_o, off_l)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_decoder_ids_are_not_looked_at_without_a_start_id(dtype):
    """decoder_start_id == HUTK_NO_TOKEN: d_decoder_ids may be anything.  Here it is the address of the input ids, real
    memory that an overlap check would refuse and a store would spoil: the call succeeds, the ids are as they were, and
    the other five outputs are those of a call without a decoder row."""
    from hutoken_amd import _capi
    ids_t, mask_t, _lengths, plan_t = rule_rows(dtype, L=260, n=6)
    before = host(ids_t).copy()
    want = reference(before, host(mask_t), host(plan_t), seed=5, density=0.3, start=None)
    rc, outs, clean = raw_span(plan_t, ids_t, mask_t, 260, 260, ids_t.element_size(), seed=5, th=S.thresholds(0.3), start=_capi.NO_TOKEN,
                               dec_over=ids_t)
    assert rc == 0 and clean and same(host(ids_t), before)
    for name, g, w in zip(NAMES[:5], outs, want):
        assert same(g, w), name
    assert (outs[5] == 77).all()  # (the guarded decoder buffer was not handed over: nothing wrote to it)


# ---- hostile plans ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("L", [8, 7, 261])
def test_hostile_plans_and_masks_stay_inside_their_buffers(L, dtype):
    """A plan and a mask are a caller's tensors.  Whatever they hold -- the mask bytes here are random and agree with no
    plan -- nothing is written outside the six outputs: HUTK_E_ARG where the restatement says so, guard bands left as
    they were, and every row as the restatement has it."""
    import hutoken_amd
    rng = np.random.default_rng(18)
    big = 2**62
    whole = min(L, 40)
    sound = [[0, 0, 3, 4, 1, 2, 2, 5], [1, 0, 0, 0, 0, 0, 0, 0], [2, 0, 40 - whole, whole, 0, 0, 0, whole], [3, 0, 0, L, 0, 0, 0, L]]
    defects = {"src_a behind the words": [0, 0, 38, 4, 0, 0, 0, 4],
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
    no_defect_here = ("src_a behind the words", "src_a negative", "src_b far away", "src_a at the lowest value")  # (no words are read)
    width = 4 if dtype == "int32" else 8
    for name, rows in [("sound", sound)] + [(k, [v]) for k, v in defects.items()] + [("all", sound + list(defects.values()))]:
        plan = np.array(rows, dtype=np.int64)
        n = len(plan)
        ids = rng.integers(100, 50000, size=(n, L)).astype(dtype)
        mask = (rng.random((n, L)) < 0.8).astype(np.uint8) * rng.integers(1, 256, size=(n, L)).astype(np.uint8)
        d_plan, d_ids, d_mask = dev(plan), dev(ids), dev(mask)
        for density, probs, L_tgt in ((0.5, None, L), (1.0, [0.5, 0.5], 3)):
            want = reference(ids, mask, plan, seed=5, density=density, probs=probs, start=5, L_tgt=L_tgt)
            assert want[6] == (name != "sound" and name not in no_defect_here), name
            rc, outs, clean = raw_span(d_plan, d_ids, d_mask, L, L_tgt, width, seed=5, th=S.thresholds(density, span_length_probs=probs))
            assert rc == (E_ARG if want[6] else 0) and clean, (L, name, rc)
            for what, g, w in zip(NAMES, outs, want):
                assert same(g, w), (L, name, what)
        call = lambda: hutoken_amd.corrupt_spans(d_ids, d_mask, d_plan, sentinel_first=FIRST, seed=5, noise_density=0.5, check=True)  # noqa: E731
        if want[6]:
            with pytest.raises(ValueError, match="row_plan"):
                call()
        else:
            call()


# ---- the round trip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", WIDTHS)
def test_round_trip_of_the_gpus_own_outputs(dtype):
    """Every sentinel of a corrupted row replaced by the ids behind it in the target gives the real columns of the row it
    was made from: from nothing but the outputs."""
    import hutoken_amd
    ids_t, mask_t, _lengths, plan_t = rule_rows(dtype, L=300, n=40, padding_side="left")
    L = ids_t.shape[1]
    out, _m, labels, in_len, tgt_len = (host(x) for x in hutoken_amd.corrupt_spans(ids_t, mask_t, plan_t, sentinel_first=FIRST, seed=9,
                                                                                   noise_density=0.3, max_target_length=2 * L))
    ids, mask = host(ids_t), host(mask_t)
    for r in range(len(ids)):
        target = labels[r, :tgt_len[r]].tolist()
        spans, key = {}, None
        for x in target:
            if x > FIRST - 100:
                key = x
                spans[key] = []
            else:
                spans[key].append(x)
        row = []
        for x in out[r, :in_len[r]].tolist():
            row += spans.pop(x) if x > FIRST - 100 else [x]
        assert not spans and row == ids[r][mask[r] != 0].tolist(), r
    assert (tgt_len > 20).all()


# ---- end to end -------------------------------------------------------------------------------------------------------
def init():
    import hutoken_amd
    from hutoken_amd import data
    vp, sp, _kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, is_byte_encoder=True)
    return hutoken_amd


def test_batch_encode_span_corruption():
    import torch
    hutoken = init()
    texts = FC.NER_TEXTS + FC.CONTEXTS + FC.short_texts(30)
    tpl = dict(eos_id=50256, pad_id=50255)
    kw = dict(sentinel_first=50354, seed=77, noise_density=0.3, target_eos_id=50256, decoder_start_id=50255)
    assert torch.cuda.current_stream().cuda_stream == 0
    for L, side, dtype in ((24, "right", "int32"), (None, "left", "int64")):
        ids_t, mask_t, _lengths, plan_t = hutoken.batch_encode_padded(texts, L, padding_side=side, dtype=dtype, return_plan=True, **tpl)
        two = hutoken.corrupt_spans(ids_t, mask_t, plan_t, pad_id=50255, max_target_length=8, **kw)
        one = hutoken.batch_encode_span_corruption(texts, L, padding_side=side, dtype=dtype, max_target_length=8, sides="a", check=True, **tpl, **kw)
        assert len(one) == 6 and all(same(host(a), host(b)) for a, b in zip(one, two))
        want = S.span_corrupt_ref(host(ids_t), host(mask_t), host(plan_t), seed=77, sentinel_first=50354, target_eos_id=50256,
                                  decoder_start_id=50255, pad_id=50255, max_target_len=8, **S.thresholds(0.3))
        assert not want[6] and all(same(host(a), b) for a, b in zip(one, want))
        assert (host(one[2]) >= 50255).any() and (host(one[4]) > 8).any() and (host(one[4]) <= 8).any()
        st = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(st):
            on_side = hutoken.batch_encode_span_corruption(texts, L, padding_side=side, dtype=dtype, max_target_length=8, **tpl, **kw)
            torch.cuda.synchronize()
        assert all(same(host(a), host(b)) for a, b in zip(one, on_side))
    with pytest.raises(TypeError, match="plan"):
        hutoken.batch_encode_span_corruption(texts, 24, return_plan=True, **kw)
    none = hutoken.batch_encode_span_corruption(texts, 24, sides="b", **tpl, **kw)  # a padded row has no B side: nothing is noise
    plain = hutoken.batch_encode_padded(texts, 24, **tpl)
    assert same(host(none[0]), host(plain[0])) and (host(none[4]) == 1).all()
