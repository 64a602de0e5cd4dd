"""The restatement of the Unigram seed rule (tests/unigram_seed_ref.py) on one corpus worked by hand, and UnigramSeeder's refusals.
No device.

The corpus, Metaspace shape: "the she", "aaaa", "xyz xyw", and "the" three times more.  Unique words (n_w): " the" (4), " she" (1),
" aaaa" (1), " xyz" (1), " xyw" (1), the space standing for U+2581.
  characters   ' ' 8, h 5, e 5, t 4 (weighted: " the" counts four times), a 4, y 2, x 2, z 1, w 1, s 1 -- by (count, c) descending
  "he"         twice (each unique word once: freq is not weighted), END behind it both times: no candidate
  " x"         always followed by y: no candidate; its extension " xy" is followed by z and by w: freq 2, score 6; "xy": score 4
  "aa"         three overlapping occurrences in "aaaa", followers a, a, END: freq 3, score 6; "aaa": freq 2, followers a, END, score 6
  " a", " aa", " aaa": followed by a alone; every string that ends its words alone (" the", "she", "aaaa", ..): END alone
So the candidates by (score, s) descending are "aaa" 6, "aa" 6, " xy" 6, "xy" 4; with 13 lines the cut falls inside the tie at 6."""
import math

import pytest

import unigram_seed_ref as S

DOCS = ["the she", "aaaa", "xyz xyw", "the", "the", "the"]
CHARS = [("▁", 8), ("h", 5), ("e", 5), ("t", 4), ("a", 4), ("y", 2), ("x", 2), ("z", 1), ("w", 1), ("s", 1)]


def test_the_restatement_on_the_hand_worked_corpus():
    import hutoken_amd as H
    assert hasattr(H, "UnigramSeeder")  # (what the restatement restates)
    count, freq, followers = S.tables(S.unique_words(DOCS))
    assert count[b"t"] == 4 and freq[b"he"] == 2 and followers[b"he"] == {None} and followers[b" x"] == {b"y"}
    assert freq[b"aa"] == 3 and followers[b"aa"] == {b"a", None}
    for size, subs in ((1_000_000, [("aaa", 6), ("aa", 6), ("▁xy", 6), ("xy", 4)]), (13, [("aaa", 6), ("aa", 6)]), (11, [])):
        lines = CHARS + subs
        total = sum(c for _s, c in lines)
        got = S.seed(DOCS, size)
        assert [p for p, _s in got] == ["<unk>"] + [s for s, _c in lines] and got[0][1] == 0.0
        assert all(abs(g - math.log(c / total)) <= 1e-12 for (_p, g), (_s, c) in zip(got[1:], lines))
    assert [p for p, _s in S.seed(DOCS, max_piece_length=2)] == ["<unk>"] + [s for s, _c in CHARS] + ["aa", "xy"]


@pytest.mark.parametrize("kwargs,error", [(dict(seed_size=1), ValueError), (dict(seed_size=True), TypeError), (dict(seed_size=1e6), TypeError),
                                          (dict(max_piece_length=0), ValueError), (dict(max_piece_length=17), ValueError),
                                          (dict(max_piece_length="16"), TypeError), (dict(unk_token=b"<unk>"), TypeError),
                                          (dict(table_slots=48), ValueError)])
def test_refusals_come_before_any_device_call(kwargs, error):
    import hutoken_amd as H
    assert "UnigramSeeder" in H.__all__ and "UnigramSeeder" in H.__doc__
    seeder = H.UnigramSeeder()
    with pytest.raises(error):
        seeder.pieces(**kwargs)
    assert seeder._h is None  # (no handle: nothing reached the device)
    if "seed_size" in kwargs or "max_piece_length" in kwargs:
        with pytest.raises(error):
            H.train_unigram(["a b"], None, 10, **kwargs)
    with pytest.raises(ValueError):
        H.UnigramSeeder(prepend_scheme="never", whitespace_split=True)
    with pytest.raises(TypeError):
        seeder.add_texts("not a list")
