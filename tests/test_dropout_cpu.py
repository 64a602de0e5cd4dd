"""BPE-dropout without a GPU: the restatement on a hand-worked word and against its closed form, refusals, exports."""
import math

import pytest

import dropout_ref as R

ABC = R.StringModel({b"a": 0, b"b": 1, b"c": 2, b"ab": 3, b"bc": 4, b"abc": 5})


@pytest.mark.parametrize("gone,want", [
    (set(), [5]),                      # ab (rank 3) before bc (rank 4), then ab + c
    ({(0, 0)}, [5]),                   # ab is dropped at step 0: bc is applied, and a + bc at step 1
    ({(0, 0), (0, 1)}, [0, 4]),        # ... unless a + bc is dropped at step 1: no candidate is left
    ({(0, 0), (1, 0)}, [0, 1, 2]),     # both candidates of step 0 are dropped: the word is finished as it stands
    ({(1, 0), (0, 1)}, [3, 2]),        # bc's drop changes nothing at step 0; ab + c is dropped at step 1
])
def test_a_hand_worked_word(gone, want):
    # the word stands at offset 7 of its document: a candidate is named by the offset of its left unit's first byte
    assert R.encode_word(ABC, b"abc", 7, lambda offs, t: [(o - 7, t) in gone for o in offs]) == want


MODEL = R.StringModel({b"a": 0, b"b": 1, b"ab": 2, b"ba": 3, b"aba": 4, b"bab": 5, b"abab": 6})


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_the_distribution_of_one_word(p):
    import numpy as np
    from targets_ref import philox4x32_10
    word, N = b"abab", 65536
    want = R.distribution(MODEL, word, p)
    assert abs(sum(want.values()) - 1) < 1e-12 and len(want) >= 6
    assert R.distribution(MODEL, word, 0.0) == {(6,): 1.0} and R.distribution(MODEL, word, 1.0) == {(0, 1, 0, 1): 1.0}
    # every draw the word can ask for, in one call: [document, offset 3 .. 6, step 0 .. 3]
    d, o, t = np.arange(N, dtype=np.uint64)[:, None, None], 3 + np.arange(4)[None, :, None], np.arange(4)[None, None, :]
    gone = (philox4x32_10((d & np.uint64(R.M32), d >> np.uint64(32), o, (t << 4) | R.PURPOSE), (2024, 0))[0] < R.threshold(p)).tolist()
    got = {}
    for g in gone:
        ids = tuple(R.encode_word(MODEL, word, 3, lambda offs, step: [g[x - 3][step] for x in offs]))
        got[ids] = got.get(ids, 0) + 1
    assert set(got) <= set(want)
    for ids, q in want.items():
        assert abs(got.get(ids, 0) - N * q) <= 5 * math.sqrt(N * q * (1 - q)) + 1, (ids, got.get(ids, 0), N * q)


@pytest.mark.parametrize("kw,exc", [(dict(dropout=0.5), ValueError), (dict(dropout=-0.1, seed=1), ValueError),
                                    (dict(dropout=1.5, seed=1), ValueError), (dict(dropout=float("nan"), seed=1), ValueError),
                                    (dict(dropout=0.5, seed=1, first_doc=-1), ValueError), (dict(dropout=0.5, seed=-1), ValueError),
                                    (dict(dropout="0.5", seed=1), TypeError), (dict(dropout=0.5, seed=1.5), TypeError)])
def test_refusals_before_any_device_call(kw, exc):
    import hutoken_amd
    with pytest.raises(exc):  # (before the context and the tensors are looked at: None stands for them)
        hutoken_amd.encode_packed_device(None, None, **kw)
    with pytest.raises(exc):
        hutoken_amd.batch_encode_dropout(["a"], kw["dropout"], kw.get("seed"), kw.get("first_doc", 0))


def test_exports():
    import inspect

    import hutoken_amd
    from hutoken_amd import _capi
    assert {"encode_dropout", "batch_encode_dropout"} <= set(hutoken_amd.__all__)
    assert "hutk_encode_dropout_batch_device" in _capi.EXPORTS and hasattr(_capi.load(), "hutk_encode_dropout_batch_device")
    sig = inspect.signature(hutoken_amd.encode_packed_device).parameters
    assert list(sig) == ["d_bytes", "d_offsets", "check", "dropout", "seed", "first_doc"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("dropout", "seed", "first_doc")) and sig["seed"].default is None
    assert _capi.dropout_info()["max_word_bytes"] == R.MAX_WORD_BYTES
