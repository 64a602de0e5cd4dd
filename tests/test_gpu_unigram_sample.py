"""Unigram subword regularisation on the GPU (k_ug_sample) against unigram_sample_ref: exact wherever the reference's
draws stay 1e-9 from a boundary (a few ulp of exp and log over at most 256 candidates move a sum far less than 1e-12).  Needs an MI355X."""
import math

import pytest

import unigram_cases as UC
import unigram_ref as R
import unigram_sample_ref as S
from test_gpu_unigram import M, MB, _chunk, _dev, _give_the_workspaces_back, _to_device, _ug  # noqa: F401 (the fixture closes the handles)

pytestmark = pytest.mark.gpu
# a start of "a" * k has min(k, 17) candidates: 7, 8, 9, 16, 17 are the edges of a trip of 8 lanes; "x", "文": unknown; ring 32
SMALL = tuple([("<unk>", 0.0), (M, -0.5), (M + "a", -1.25), ("b", -1.5), ("ab", -2.25), ("ba", -2.0), ("é", -1.0), ("中", -1.75), ("é中", -2.5),
               ("😀", -3.0), ("a😀", -3.25)] + [("a" * k, -0.625 * k - 0.25 * (k % 3)) for k in range(1, 18)])
# a key past 63 bytes (bit 63 of the length mask) and one at the 256-byte bound: a ring of 512 positions, 8 groups
VOCABS = {"small": (SMALL, 32), "long": (SMALL + (("ab" * 50, -7.0), ("ab" * 128, -9.5)), 512)}  # name -> (vocabulary, the ring)


def _docs(ring):
    def pad(n):  # n bytes of the words " ab", the last one longer
        return b" ab" * (n // 3) + b"b" * (n % 3)
    C, word = _chunk(), b" aabbaabbaab"  # 12 bytes: the first ends exactly on the first chunk edge (the document is the batch's first
    docs = [pad(C - 12) + word + pad(C - 5) + word + b" ab a", b""]  # and under never_collapse the fold moves nothing), the second crosses the next
    docs += [b"a" * k for k in (1, 7, 8, 9, 16, 17, 18, 40)] + [b"", b"", b"ab" * 128 + b"a" * 20 + b"ab" * 50]
    docs += [(b"ab" * (2 * ring))[:n] for n in (ring - 2, ring - 1, ring, ring + 1, 3 * ring + 5)]
    docs += ["é中 aé中😀a 😀é a😀 文é中文".encode(), b"\x80a \xe4\xb8a a\xffb \xf0\x9f\x98 \xc3", "é".encode()[:1] + "中".encode()]
    return docs + [b"xxab abxxab abxx xx x " + MB + b"x  a\tb", b"", b" ", b"ba ab aab baab"]


@pytest.mark.parametrize("name,shape,alpha,seed", [("small", shape, alpha, 11) for shape in sorted(UC.SHAPES) for alpha in (0, 0.1, 1, 16, -1)]
                         + [("long", "never_collapse", 0.1, 12), ("long", "metaspace", 1, 13), ("long", "whitespace_split", -1, 14)])
def test_exact_against_the_restatement(name, shape, alpha, seed):
    vocab, docs = VOCABS[name][0], _docs(VOCABS[name][1])
    want = S.sample_docs(R.Vocab(vocab, 0), docs, alpha, seed, 5, **UC.SHAPES[shape])
    assert want[3] >= 1e-9, "a draw of this seed lies within 1e-9 of a boundary: take another seed"
    ids, oo, wids = _ug(vocab, 0, shape).encode_packed_device(*_to_device(docs), return_word_ids=True, alpha=alpha, seed=seed, first_doc=5)
    assert oo.tolist() == want[1] and ids.tolist() == want[0] and wids.tolist() == want[2]


def test_the_empty_batch_and_batch_independence():
    ug, docs = _ug(SMALL, 0), _docs(32)
    ids, oo = ug.encode_packed_device(*_to_device([]), alpha=0.5, seed=3)
    assert ids.numel() == 0 and oo.tolist() == [0]
    whole = ug.encode_packed_device(*_to_device(docs), return_word_ids=True, alpha=0.5, seed=3)
    for k in (1, 4, len(docs) - 1):  # the documents from k on, numbered from k: the tail of the whole batch
        ids, oo, wids = ug.encode_packed_device(*_to_device(docs[k:]), return_word_ids=True, alpha=0.5, seed=3, first_doc=k)
        at = whole[1][k].item()
        assert ids.tolist() == whole[0][at:].tolist() and wids.tolist() == whole[2][at:].tolist() and oo.tolist() == (whole[1][k:] - at).tolist()


@pytest.mark.parametrize("alpha", [0, 1])
def test_the_distribution_of_one_word(alpha):
    word, N = b"abaxab", 65536  # ("a b a" | "ab a" | "a ba") <unk> ("a b" | "ab"): six segmentations
    want = {}
    for ids, p in S.segmentations(R.Vocab(SMALL, 0), word, alpha):
        want[ids] = want.get(ids, 0.0) + p
    ids, oo = _ug(SMALL, 0, "never_collapse").encode_packed_device(*_to_device([word] * N), alpha=alpha, seed=2024)
    flat, oo = ids.tolist(), oo.tolist()
    got = [tuple(flat[oo[i]:oo[i + 1]]) for i in range(N)]
    assert len(want) == 6 and set(got) <= set(want)
    for seg, p in want.items():
        assert abs(got.count(seg) - N * p) <= 5 * math.sqrt(N * p * (1 - p)) + 1, (seg, got.count(seg), N * p)


def test_plumbing():
    ug, texts = _ug(SMALL, 0), ["aaa ab", "", "é中 xab"]
    db, do = _to_device([t.encode() for t in texts])
    plain = ug.encode_packed_device(db, do, return_word_ids=True)
    assert all(a.tolist() == b.tolist() for a, b in zip(plain, ug.encode_packed_device(db, do, return_word_ids=True, alpha=None)))
    ids, oo = ug.encode_packed_device(db, do, alpha=0.3, seed=7, first_doc=2)
    rows = ug.batch_encode(texts, alpha=0.3, seed=7, first_doc=2)
    assert [t for r in rows for t in r] == ids.tolist() and [len(r) for r in rows] == (oo[1:] - oo[:-1]).tolist()
    assert ug.encode(texts[2], alpha=0.3, seed=7, first_doc=4) == rows[2]
    raw = (db.data_ptr(), do.data_ptr(), 3, db.numel(), 0, 0, do.data_ptr())  # (the C entry refuses before it reads or writes anything)
    for kw, exc, c_exc in ((dict(alpha=0.3), TypeError, None), (dict(alpha=math.inf, seed=1), ValueError, ValueError),
                           (dict(alpha=0.3, seed=1, first_doc=-1), ValueError, TypeError)):  # (HUTK_E_VALUE; HUTK_E_ARG is TypeError)
        with pytest.raises(exc):
            ug.encode_packed_device(db, do, **kw)
        with pytest.raises(exc):
            ug.batch_encode(texts, **kw)
        if c_exc:
            with pytest.raises(c_exc):
                ug._handle(_dev()).sample_device(*raw, kw["alpha"], kw["seed"], kw.get("first_doc", 0))
