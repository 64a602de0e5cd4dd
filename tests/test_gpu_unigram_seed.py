"""UnigramSeeder on the GPU (csrc/hutk_unigram_seed.h) against tests/unigram_seed_ref.py: the pieces and their order
exactly, the scores to 1e-12 absolute (both sides take the logarithms of the same integers).  Needs an MI355X."""
import random

import pytest

import unigram_cases as UC
import unigram_ref as R
import unigram_seed_ref as S
import unigram_train_ref as T
from test_gpu_unigram import M, _to_device
from test_gpu_unigram_train import _fit_corpus

pytestmark = pytest.mark.gpu
TILE, HALO, CHUNK = 2048, 64, 4096


def _edge_word():
    """One word of 5000 folded bytes (longer than a tile and than a chunk) that the first add puts at arena position 1: sixteen 4-byte
    characters start on the first tile's last byte and end on the halo's last byte, with z behind them."""
    rng = random.Random(5)
    head = "".join(rng.choice("abc") for _ in range(TILE - 1 - 2))  # arena: 0x00, the U+2581, then the head up to position TILE - 2
    word = head + "😀" * 16 + "z" + "é中" * 40
    return word + "".join(rng.choice("abc") for _ in range(5000 - 1 - len(word.encode())))


def _edge_docs():
    rng = random.Random(6)
    docs = [("😀" * 16 + "y " + "中文" * 9 + " " + M + "q" + M + M + "r").encode(), b"a\xff\xfeb \xe4\xb8 ab\x00ab\x00 \xf0\x9f\x98 ab", b"\x00", b""]
    long = "abcdefghi中" * 9  # words past 64 bytes are a wavefront's: the same one again in its batch, and one that differs in its last byte
    docs += [(long + " " + long + "x " + long).encode(), (long + "y").encode(), _edge_word().encode()]  # (and the edge word, in a later add)
    docs += [" ".join(rng.choice(["ab", "abab", "aé", "中a", "b", "😀b"]) for _ in range(rng.randint(1, 30))).encode() for _ in range(300)]
    return docs


def _check(seeder, docs, shape="metaspace", **kwargs):
    got = seeder.pieces(**kwargs)
    want = S.seed(docs, **{k: v for k, v in kwargs.items() if k != "table_slots"}, **UC.SHAPES[shape])
    assert [p for p, _s in got] == [p for p, _s in want]
    assert all(abs(a - b) <= 1e-12 for (_p, a), (_q, b) in zip(got, want))
    return want


@pytest.mark.parametrize("shape", sorted(UC.SHAPES))
def test_every_shape_and_two_halves(shape):
    import hutoken_amd as H
    docs = [R.to_bytes(d) for d in UC.corpus(90, 11) + UC.random_docs(random.Random(shape), 200)]
    assert sum(map(len, docs)) > CHUNK
    one, two = H.UnigramSeeder(**UC.SHAPES[shape]), H.UnigramSeeder(**UC.SHAPES[shape])
    one.add(_to_device(docs))
    two.add([_to_device(docs[:100]), _to_device([])]).add(_to_device(docs[100:]))
    words = S.unique_words(docs, **UC.SHAPES[shape])
    assert one.n_words == two.n_words == len(words) and one.n_occurrences == two.n_occurrences == sum(words.values())
    assert sorted(one.words()[3].tolist()) == sorted(words.values())
    want = _check(one, docs, shape)
    assert two.pieces() == one.pieces() and len(want) > 100
    subs = [s for _p, s in want if len(_p) > 1][1:]
    cut = next(i for i in range(len(subs) - 1) if subs[i] == subs[i + 1])  # a seed_size that cuts inside a tie group
    for size, length in ((len(want) - len(subs) + cut + 1, 16), (1_000_000, 2), (1_000_000, 1), (len(want) - len(subs), 16)):
        _check(one, docs, shape, seed_size=size, max_piece_length=length)
    with pytest.raises(ValueError, match="characters"):
        one.pieces(seed_size=3)


def test_tile_chunk_and_halo_edges_and_odd_bytes():
    import hutoken_amd as H
    first, docs = _edge_word(), _edge_docs()
    assert len(first.encode()) + 1 == 5000 and first.encode()[TILE - 3:TILE - 3 + 64] == "😀".encode() * 16
    seeder = H.UnigramSeeder().add_texts([first, first]).add(_to_device(docs))
    arena, starts, lengths, counts = seeder.words()
    assert (starts[0].item(), lengths[0].item(), counts[0].item()) == (1, 5000, 3) and bytes(arena[TILE - 1:TILE - 1 + HALO].tolist()) == "😀".encode() * 16
    want = _check(seeder, [first.encode()] * 2 + docs)
    assert "😀" * 16 in [p for p, _s in want] and "\udcff" in [p for p, _s in want]
    _check(seeder, [first.encode()] * 2 + docs, table_slots=16)  # the counting pass doubles its table
    assert seeder._h.info()["substring_slots"] >= 64


def test_the_word_table_grows_and_a_hot_word():
    import hutoken_amd as H
    rng = random.Random(7)
    docs = [" ".join("".join(rng.choice("abcdefgh") for _ in range(rng.randint(1, 9))) for _ in range(40)).encode() for _ in range(150)]
    seeder = H.UnigramSeeder(prepend_scheme="never").add(_to_device(docs)).add(_to_device([b"a"] * 4096))
    assert seeder._h.info()["word_table_grows"] >= 1 and seeder.n_words > 2048
    got, want = seeder.pieces(), S.seed(docs + [b"a"] * 4096, prepend_scheme="never")
    assert [p for p, _s in got] == [p for p, _s in want] and all(abs(a - b) <= 1e-12 for (_p, a), (_q, b) in zip(got, want))
    empty = H.UnigramSeeder().add(_to_device([]))
    assert empty.pieces() == [("<unk>", 0.0)] and empty.n_words == 0


def test_train_unigram_from_the_corpus_alone():
    import hutoken_amd as H
    docs = _fit_corpus(3)  # (a corpus on which the restated fit keeps its margins with this seed: it asserts them)
    seed = S.seed(docs, 400)
    size = sum(len(p) == 1 for p, _s in seed) + 1 + 60
    want, n_top, z_top = T.fit([p for p, _s in seed], [s for _p, s in seed], 0, docs, size, **UC.SHAPES["metaspace"])
    rtol = 16 * n_top * max(1.0, z_top) * 2.0 ** -53
    batch = _to_device([d.encode() for d in docs])
    for got in (H.train_unigram(docs, None, size, seed_size=400), H.UnigramTrainer.from_corpus(batch, seed_size=400).fit(batch, size)):
        assert got._pieces == [p for p, _s in want] and got.unk_id == 0 and got.vocab_size == size
        assert all(abs(a - b) <= rtol * abs(b) + 1e-12 for a, (_p, b) in zip(got._scores, want))
