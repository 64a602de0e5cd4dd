"""tests/wide_cases.py held to its claims without a GPU: the straddler layout of every kind of block (with the boundaries
2^20 and 2^21 and a block of about 70 000 bytes, and of the full-size text block the GPU test uses), the cap on long
words, and the premise of tests/test_gpu_wide_batches.py -- every reference gives, for three copies of a block, three
times what it gives for one."""
import numpy as np
import pytest

import decode_cases as DC
import fallback_ref as F
import norm_ref as NR
import spans_ref as S
import specials_ref as SR
import wide_cases as W

LO, HI = 2 ** 20, 2 ** 21
SMALL = W.choose_length(70001, LO, HI, 2048, 4200)
EOT, EOT_ID = W.EOT, W.EOT_ID


@pytest.fixture(scope="module")
def small():
    return {kind: W.build(kind, SMALL, LO, HI, rich=False) for kind in W.KINDS}


def test_block_length_is_odd_and_leaves_room_for_the_zones():
    assert SMALL % 2 == 1 and 70001 <= SMALL < 80000
    L = W.choose_length(16 * 2 ** 20 + 1, W.B31, W.B32, 2 ** 20, 2 ** 20)
    assert L % 2 == 1 and 16 * 2 ** 20 < L < 32 * 2 ** 20
    for p in (W.B31 % L, W.B32 % L):
        assert 2 ** 20 <= p <= L - 2 ** 20
    assert abs(W.B31 % L - W.B32 % L) >= 2 ** 21


@pytest.mark.parametrize("kind", W.KINDS)
def test_straddler_layout(small, kind):
    b = small[kind]
    assert b.L == SMALL and int(b.offs[-1]) == SMALL and b.p_lo == LO % SMALL and b.p_hi == HI % SMALL
    W.check_layout(b)
    offs = set(b.offs.tolist())
    assert b.p_lo + 960 in offs and b.p_hi + 960 in offs
    assert not (b.data == 0).any()
    if kind != "norm":
        assert b.data[b.p_hi - 1 + 1920] >> 4 == 0xE  # the lead byte of a three-byte character
    # the layout check is no formality: a block shifted by one byte fails it
    moved = W.Block(kind, [b"x"] + b.docs[:-1] + [b.docs[-1][:-1]], LO, HI)
    assert moved.L == SMALL
    with pytest.raises(AssertionError):
        W.check_layout(moved)


def test_full_size_text_block():
    """the block of the GPU test: the layout at 2^31 and 2^32, every exception list, the over-long word, the cap"""
    L = W.choose_length(16 * 2 ** 20 + 1, W.B31, W.B32, 2 ** 20, 2 ** 20)
    b = W.build("text", L, W.B31, W.B32)
    assert b.L == L and b.p_lo == W.B31 % L and b.p_hi == W.B32 % L
    share = W.long_share(b)
    assert share <= W.LONG_SHARE, share
    sizes = np.array([e - s for s, e in W.runs(b, 49)])
    for lo, hi in ((49, 64), (65, 128), (129, 256), (257, 512), (513, 1024), (1025, 2046), (2047, 262144)):
        assert ((sizes >= lo) & (sizes <= hi)).any(), (lo, hi)
    assert (sizes >= W.OVERLONG).sum() == 1
    lens = np.diff(b.offs)
    assert (lens == 0).sum() >= 4 and (lens == 1).sum() >= 4
    assert W.copies_cross(b.L, W.B31) * b.L >= W.B31 + 2 ** 26 and W.copies_cross(b.L, W.B32) * b.L >= W.B32 + 2 ** 26


def test_repeated_offsets_and_sides():
    offs = np.array([0, 3, 3, 10], dtype=np.int64)
    assert W.repeated_offsets(offs, 10, 3).tolist() == [0, 3, 3, 10, 13, 13, 20, 23, 23, 30]
    assert W.side(2 ** 31 - 1) == "below 2^31" and "[2^31, 2^32)" in W.side(2 ** 31) and "above 2^32" in W.side(2 ** 32)
    assert W.copies_cross(10, 95, extra=5) == 10 and W.copies_cross(10, 96, extra=5) == 11


def test_comparison_names_copy_position_and_side():
    """assert_rows and assert_offsets on host tensors: silent when the batch is R times the row, and a single wrong
    element is found in whichever slice it lies, with its copy, its byte position and the side of the boundary."""
    import torch
    Lb, T, R = 1001, 7, 5000  # (5000 copies of 1001 bytes: positions up to 5 005 000; a slice holds two copies)
    row = torch.arange(T, dtype=torch.int32) * 3
    got = row.repeat(R)
    where = lambda r, j: r * Lb + 100 * j  # noqa: E731
    W.assert_rows(got, row, R, "ids", where, Lb, slice_elems=2 * T)
    got[4321 * T + 5] += 1
    got[4800 * T] += 1  # (a later one: not the one reported)
    with pytest.raises(AssertionError) as e:
        W.assert_rows(got, row, R, "ids", where, Lb, slice_elems=2 * T)
    msg = str(e.value)
    assert "element 5 of copy 4321 " in msg and "byte position %d = 4321 * 1001 + 500" % (4321 * Lb + 500) in msg and "below 2^31" in msg
    assert ": 16, the reference has 15" in msg
    with pytest.raises(AssertionError, match="35 elements, 4 copies of 7 expected"):
        W.assert_rows(got[:35], row, 4, "ids", where, Lb)
    oo_b = np.array([0, 3, 3, 10], dtype=np.int64)
    oo = torch.from_numpy(W.repeated_offsets(oo_b, 10, R))
    W.assert_offsets(oo, oo_b, R, "offsets", where, Lb, slice_elems=4)
    oo[3 * 77 + 2] -= 1
    with pytest.raises(AssertionError, match="element 2 of copy 77 "):
        W.assert_offsets(oo, oo_b, R, "offsets", where, Lb, slice_elems=4)
    oo[3 * 77 + 2] += 1
    oo[-1] += 1
    with pytest.raises(AssertionError, match="the total is 50001, 5000 copies of 10 expected"):
        W.assert_offsets(oo, oo_b, R, "offsets", where, Lb)
    # the side in the message is that of the position, whatever the element's own index
    with pytest.raises(AssertionError, match=r"wraps as uint32"):
        W.assert_rows(torch.tensor([1, 2, 1, 3]), torch.tensor([1, 2]), 2, "x", lambda r, j: 2 ** 32 + 5, Lb)
    with pytest.raises(AssertionError, match=r"negative as int32"):
        W.assert_rows(torch.tensor([1, 2, 1, 3]), torch.tensor([1, 2]), 2, "x", lambda r, j: 2 ** 31, Lb)


# ---- the premise: R copies of a block give R times the block's result ---------------------------------------------------
def _three(b):
    return np.tile(b.data, 3), W.repeated_offsets(b.offs, b.L, 3)


def _assert_tripled(one, three, totals=None):
    """(flat values, offsets, status) of the block and of its three copies"""
    v1, o1, s1 = one
    v3, o3, s3 = three
    T = int(o1[-1])
    assert np.array_equal(np.asarray(v3), np.tile(np.asarray(v1), 3 if np.asarray(v1).ndim == 1 else (3, 1)))
    assert np.array_equal(o3, W.repeated_offsets(o1, T, 3))
    assert np.array_equal(np.asarray(s3), np.tile(np.asarray(s1), 3))


@pytest.fixture(scope="module")
def oracles(oracle_mod):
    from hutoken_amd import data
    out = {}
    for name in ("VG", "VL"):
        vp, sp, kw = data.vocab_files(name)
        out[name] = (oracle_mod.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"]), kw["is_byte_encoder"], (vp, sp, kw))
    return out


@pytest.mark.parametrize("name,kind", [("VG", "text"), ("VL", "chars"), ("VG", "cjk"), ("VG", "dense")])
def test_oracle_is_periodic(small, oracles, name, kind):
    orc = oracles[name][0]
    b = small[kind]
    one = orc.encode_packed(b.data, b.offs, 4)
    _assert_tripled(one, orc.encode_packed(*_three(b), 4))
    assert len(one[0]) > b.L // 8
    if name == "VL":
        assert not one[2].any()  # (valid UTF-8 throughout: a character-mode context refuses anything else)


def test_decode_ref_is_periodic(small, oracles):
    orc, _is_byte, files = oracles["VG"]
    ref = DC.shipped_vocab_ref(files)
    b = small["text"]
    ids, oo, _st = orc.encode_packed(b.data, b.offs, 4)
    text1, to1 = ref.decode_packed(ids, oo)
    text3, to3 = ref.decode_packed(np.tile(ids, 3), W.repeated_offsets(oo, int(oo[-1]), 3))
    zeros = np.zeros(len(b.docs), dtype=np.int32)
    _assert_tripled((text1, to1, zeros), (text3, to3, np.tile(zeros, 3)))
    assert np.array_equal(text1, b.data) and np.array_equal(to1, b.offs)  # (no document of the small block is cut)


@pytest.mark.parametrize("name", ["VG", "VL"])
@pytest.mark.parametrize("unit", ["byte", "char"])
def test_spans_ref_is_periodic(small, oracles, name, unit):
    orc, is_byte, files = oracles[name]
    b = small["text" if is_byte else "chars"]
    # (VG through decode_ref's tables, as the GPU test has them: the oracle decodes a GPT-2 token in 0.1 ms)
    tt = W.RefTokenText(DC.shipped_vocab_ref(files)) if name == "VG" else S.TokenText(orc)
    ids, oo, _st = orc.encode_packed(b.data, b.offs, 4)
    if name == "VG":
        slow = S.TokenText(orc)
        for i in np.unique(ids)[::50].tolist():
            assert tt.first(i) == slow.first(i) and tt.rest(i) == slow.rest(i), i
    sp1, st1 = S.batch(tt, b.data, b.offs, ids, oo, is_byte, unit, np.int64)
    data3, offs3 = _three(b)
    sp3, st3 = S.batch(tt, data3, offs3, np.tile(ids, 3), W.repeated_offsets(oo, int(oo[-1]), 3), is_byte, unit, np.int64)
    _assert_tripled((sp1, oo, st1), (sp3, W.repeated_offsets(oo, int(oo[-1]), 3), st3))
    assert not st1.any()


@pytest.mark.parametrize("form", ["NFC", "NFKD"])
def test_norm_ref_is_periodic(small, form):
    b = small["norm"]
    out1, oo1, ch1 = NR.reference(form, b.docs)
    out3, oo3, ch3 = NR.reference(form, b.docs * 3)
    _assert_tripled((out1, oo1, ch1), (out3, oo3, ch3))
    assert ch1.any() and not ch1.all()


def test_markers_and_unknown_characters_lie_across_both_boundaries(small):
    """marked() and with_unknowns(): lengths and offsets stay, a marker runs from p - 8 to p + 5 and an unknown
    character from p - 1 to p + 2 at p_lo and at p_hi, every third document with room has one, a character-mode block
    stays valid UTF-8"""
    b = small["text"]
    data, at = W.marked(b)
    assert len(data) == b.L and b.p_lo - 8 in at and b.p_hi - 8 in at and len(at) > len(b.docs) // 4
    raw = data.tobytes()
    assert all(raw[s:s + len(EOT)] == EOT for s in at) and raw.count(EOT) == len(at)
    assert (data != b.data).sum() <= len(at) * len(EOT)
    c = small["chars"]
    data, at = W.with_unknowns(c)
    assert len(data) == c.L and c.p_lo - 1 in at and c.p_hi - 1 in at and len(at) > len(c.docs) // 8
    raw = data.tobytes()
    assert all(raw[s:s + 3] == W.UNKNOWN for s in at)
    for d in range(len(c.docs)):
        raw[int(c.offs[d]):int(c.offs[d + 1])].decode("utf-8")


def test_split_piece_lies_across_both_boundaries(small):
    """with_split_piece(): lengths and offsets stay; the boundary falls inside the digit run of a piece, and the presets'
    word starts differ there as their patterns say: cl100k groups the digits in threes (a start on either side), qwen2
    takes each alone, gpt2 has one word from the space in front of the run to its end."""
    import presplit_ref as PR
    b = small["text"]
    data, at = W.with_split_piece(b)
    n = len(W.SPLIT_PIECE)
    assert len(data) == b.L and b.p_lo - 9 in at and b.p_hi - 9 in at and len(at) > len(b.docs) // 4
    raw = data.tobytes()
    assert all(raw[s:s + n] == W.SPLIT_PIECE for s in at) and (data != b.data).sum() <= len(at) * n
    lo, hi = W.SPLIT_DIGITS
    assert W.SPLIT_PIECE[lo:hi].isdigit() and hi - lo == 7 and lo < 9 < hi - 1 and W.SPLIT_PIECE[lo - 1:lo] == b" "
    want = {"gpt2": [], "cl100k": [lo, lo + 3, lo + 6], "qwen2": list(range(lo, hi))}
    for preset in PR.PRESETS:
        starts, so = W.preset_words(data, b.offs, preset)
        assert so[0] == 0 and so[-1] == len(starts) and len(so) == len(b.docs) + 1 and (np.diff(starts) > 0).all()
        have = set(starts.tolist())
        for p in (b.p_lo, b.p_hi):
            s = p - 9  # where the piece begins
            assert [q - s for q in range(s + lo, s + hi) if q in have] == want[preset], (preset, p)
            assert s + 1 in have and s + lo - 1 in have and s + 18 in have  # 's, the space in front of the digits, 'll
            inside = [q for q in range(s + lo + 1, s + hi) if q in have]
            if preset == "gpt2":
                assert not inside  # one word across the boundary
            else:
                assert [q for q in inside if q < p] and [q for q in inside if q >= p]  # a start on either side of it


@pytest.mark.parametrize("preset", ["gpt2", "cl100k"])
def test_preset_ids_are_periodic_and_drop_nothing(small, oracles, oracle_mod, preset):
    """The reference of the encode under a preset: three copies give three times the block's ids, and the ids decode to
    the block's bytes, those of the words that are not valid UTF-8 included."""
    _orc, _is_byte, files = oracles["VG"]
    b = small["text"]
    data, _at = W.with_split_piece(b)
    with pytest.raises(UnicodeDecodeError):
        data.tobytes().decode("utf-8")
    starts, so = W.preset_words(data, b.offs, preset)
    ids, oo = W.preset_ids(oracle_mod, files, data, b.offs, starts, so)
    assert oo[0] == 0 and oo[-1] == len(ids) and len(oo) == len(b.docs) + 1
    text, to = DC.shipped_vocab_ref(files).decode_packed(ids, oo)
    assert np.array_equal(text, data) and np.array_equal(to, b.offs)
    data3, offs3 = np.tile(data, 3), W.repeated_offsets(b.offs, b.L, 3)
    starts3, so3 = W.preset_words(data3, offs3, preset)
    assert np.array_equal(starts3, (starts[None, :] + (np.arange(3) * b.L)[:, None]).reshape(-1))
    assert np.array_equal(so3, W.repeated_offsets(so, len(starts), 3))
    ids3, oo3 = W.preset_ids(oracle_mod, files, data3, offs3, starts3, so3)
    zeros = np.zeros(len(b.docs), dtype=np.int32)
    _assert_tripled((ids, oo, zeros), (ids3, oo3, np.tile(zeros, 3)))


def test_specials_ref_is_periodic(small, oracles):
    orc = oracles["VG"][0]
    data, offs = W.marked(small["text"])[0], small["text"].offs
    one = SR.encode(orc, data, offs, {EOT: EOT_ID})
    three = SR.encode(orc, np.tile(data, 3), W.repeated_offsets(offs, len(data), 3), {EOT: EOT_ID})
    _assert_tripled(one[:3], three[:3])
    assert one[3] > 10 and three[3] == 3 * one[3]


def test_fallback_ref_is_periodic(small, oracles):
    orc, is_byte, (vp, _sp, _kw) = oracles["VL"]
    table, _n_lines = W.byte_table(vp)
    assert len(set(table.tolist())) == 256
    b = small["chars"]
    data, at = W.with_unknowns(b)
    tt = S.TokenText(orc)
    ids, oo, _st = orc.encode_packed(data, b.offs, 4)
    assert (np.asarray(ids) == -1).sum() >= len(at)
    one = F.encode(tt, data, b.offs, ids, oo, is_byte, table)
    data3, offs3 = np.tile(data, 3), W.repeated_offsets(b.offs, b.L, 3)
    three = F.encode(tt, data3, offs3, np.tile(ids, 3), W.repeated_offsets(oo, int(oo[-1]), 3), is_byte, table)
    _assert_tripled(one, three)
    assert len(one[0]) > len(ids)
