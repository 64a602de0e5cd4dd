"""Unigram training without a GPU: the restatement (tests/unigram_train_ref.py) on a case worked by hand, its digamma against
known values, and every refusal of hutoken_amd.UnigramTrainer that needs no device."""
import math

import numpy as np
import pytest

import unigram_train_ref as T

M = "▁"
GAMMA = 0.5772156649015329


def test_the_posteriors_of_a_word_worked_by_hand():
    pieces, scores = ["<unk>", M, "a", "b", "ab", M + "a"], [0.0, -1.0, -2.0, -1.5, -3.0, -2.5]
    # "▁ab" has three paths: ▁ a b (-4.5), ▁ ab (-4), ▁a b (-4)
    p = [math.exp(-4.5), math.exp(-4.0), math.exp(-4.0)]
    total = sum(p)
    expected, stats, z_top, _abs = T.e_step(T.model(pieces, scores, 0), [(M + "ab").encode()] * 3, len(pieces))
    want = [0.0, (p[0] + p[1]) / total, p[0] / total, (p[0] + p[2]) / total, p[1] / total, p[2] / total]
    assert np.allclose(expected, 3 * np.array(want), rtol=1e-14, atol=0)
    assert stats[1] == 3 and abs(stats[0] - 3 * math.log(total)) < 1e-13 and abs(z_top + math.log(total)) < 1e-14
    # a dead "b": the unknown edge (min alive - 10 = -13) takes its place on both paths that used it, under the unknown id
    dead = [0.0, -1.0, -2.0, math.nan, -3.0, -2.5]
    q = [math.exp(-16.0), math.exp(-4.0), math.exp(-15.5)]
    expected, _stats, _z, _abs = T.e_step(T.model(pieces, dead, 0), [(M + "ab").encode()], len(pieces))
    assert np.allclose(expected, np.array([q[0] + q[2], q[0] + q[1], q[0], 0.0, q[1], q[2]]) / sum(q), rtol=1e-14, atol=0)


def test_digamma():
    # the series stops at x^-8; the next term, 511 / 122880 x^-10, is below 3.1e-11 for x - 1/2 >= 6.5
    known = {1.0: -GAMMA, 0.5: -GAMMA - 2 * math.log(2), 7.0: 1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 5 + 1 / 6 - GAMMA,
             1e6: math.log(1e6) - 0.5e-6 - 1 / 12e12}
    for x, want in known.items():
        assert abs(T.digamma(x) - want) < 1e-9, x
    assert abs(T.digamma(6.99) + 1 / 6.99 - T.digamma(7.99)) < 1e-9  # digamma(x + 1) = digamma(x) + 1 / x, across the switch at 7
    try:
        from scipy.special import digamma
    except ImportError:
        return
    for x in (0.5, 1.0, 6.99, 7.0, 1e6):
        assert abs(T.digamma(x) - float(digamma(x))) < 1e-9, x


def test_refusals_that_need_no_device():
    import hutoken_amd as H
    for seed in ([], ["<unk>", "a", "b", "a"], ["<unk>", "a", ""], ["<unk>", "a" * 257], [("<unk>", 0.0), ("a", math.inf)]):
        with pytest.raises(ValueError):
            H.UnigramTrainer(seed)
    with pytest.raises(ValueError):
        H.UnigramTrainer(["<unk>", "a"], 2)
    with pytest.raises(ValueError):
        H.UnigramTrainer(["<unk>", "a"], whitespace_split=True, prepend_scheme="never")
    with pytest.raises(TypeError):
        H.UnigramTrainer("abc")
    tr = H.UnigramTrainer(["<unk>", "a", "b", "ab", M])  # three single characters and the unknown line: 4 lines at least
    assert tr.alive == 4 and np.isnan(tr.scores[0]) and tr.scores[1] == math.log(1 / 5)
    with pytest.raises(ValueError):
        tr.fit([], 3)
    with pytest.raises(ValueError):
        H.train_unigram(["ab"], ["<unk>", "a", "b", "ab", M], 3)
    with pytest.raises(ValueError):
        tr.set_scores([0.0])
    assert [p for p, _s in T.finalize(["<unk>", "a", "b", "ab", M], [math.nan, -1.0, math.nan, -2.0, -0.5], 0, 4)] == ["<unk>", M, "a", "b"]
    assert tr.kept(np.array([np.nan, np.inf, 0.25, 0.5, -np.inf, 0.25]), 3).tolist() == [1, 2, 3]
