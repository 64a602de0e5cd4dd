"""Synthetic inputs for the word-id and answer-position kernels (csrc/hutk_features.hip: k_word_ids; csrc/hutk_collate.hip:
k_rows_answers) with their expected results: what tests/test_gpu_features_edges.py runs on the GPU and
tests/test_features_synth_cpu.py holds to its claims without one.

The kernels read no text, only arrays: a word-start bitmap with its prefix counts, text and id offsets, byte spans; a
row plan, spans and answers.  So a case is laid out from a description -- which id is a document's first, at which bit
a word starts -- and its expected result is features_ref's, per document.  Nothing here touches the package under
test."""
import random

import numpy as np

import features_ref as F

PAD_WORDS = 40  # the bitmap is int32[n_bytes // 32 + 40], as hutk_pretokenize_batch_device writes it


class WordBatch:
    """n_docs, n_bytes, n_ids; text_offs, id_offs int64[n_docs + 1]; bits int32[n_bytes // 32 + 40]; before
    int64[n_bytes // 32 + 2]; spans int64[n_ids, 2] (bytes from the document's start); words int32[n_ids]: the expected
    word ids; flagged: the documents with a word start strictly inside a token; starts: per document its word starts"""

    def __init__(self, lens, starts, spans, lead, tail, junk):
        self.lens, self.starts, self.doc_spans, self.lead, self.tail, self.junk = lens, starts, spans, lead, tail, junk
        self.n_docs = len(lens)
        self.text_offs = np.full(self.n_docs + 1, lead, dtype=np.int64)
        self.text_offs[1:] += np.cumsum(np.asarray(lens, dtype=np.int64))
        self.n_bytes = int(self.text_offs[-1]) + tail
        self.id_offs = np.zeros(self.n_docs + 1, dtype=np.int64)
        self.id_offs[1:] = np.cumsum(np.asarray([len(s) for s in spans], dtype=np.int64))
        self.n_ids = int(self.id_offs[-1])
        self.spans = np.array([ab for s in spans for ab in s], dtype=np.int64).reshape(-1, 2)
        # the bitmap: every word start, the bit at n_bytes; junk in front of the first document and behind the last
        at = [int(self.text_offs[d]) + p for d in range(self.n_docs) for p in starts[d]] + [self.n_bytes]
        if junk:
            at += list(range(0, lead)) + list(range(int(self.text_offs[-1]), self.n_bytes))
        at = np.unique(np.asarray(at, dtype=np.int64))
        words = np.zeros(self.n_bytes // 32 + PAD_WORDS, dtype=np.uint32)
        np.bitwise_or.at(words, at >> 5, np.uint32(1) << (at & 31).astype(np.uint32))
        self.bits = words.view(np.int32)
        self.before = prefix_counts(words, self.n_bytes)
        # the expected ids: features_ref, per document
        out, self.flagged = np.zeros(self.n_ids, dtype=np.int32), []
        for d in range(self.n_docs):
            w, mismatch = F.word_ids(None, spans[d], starts[d])
            out[self.id_offs[d]:self.id_offs[d + 1]] = w
            if mismatch:
                self.flagged.append(d)
        self.words = out


def prefix_counts(words, n_bytes):
    """int64[n_bytes // 32 + 2]: the set bits of the bitmap below word w (numpy population counts, a cumulative sum)"""
    n = n_bytes // 32 + 1
    per_word = np.unpackbits(np.ascontiguousarray(words[:n]).view(np.uint8)).reshape(n, 32).sum(axis=1, dtype=np.int64)
    before = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(per_word, out=before[1:])
    return before


def word_batch(docs, lead=0, tail=0, junk=True):
    """docs: a list of documents, a document a list of words, a word a list of token byte lengths (0: an empty span; a
    word has a byte at least).  The first document's text begins at byte `lead`, `tail` bytes follow the last; with junk
    every bit of those bytes is set in the bitmap, which must change nothing."""
    lens, starts, spans = [], [], []
    for doc in docs:
        at, st, sp = 0, [], []
        for word in doc:
            assert sum(word) >= 1 and min(word) >= 0, "a word has a byte at least"
            st.append(at)
            for n in word:
                sp.append((at, at + n))
                at += n
        lens.append(at)
        starts.append(st)
        spans.append(sp)
    return WordBatch(lens, starts, spans, lead, tail, junk)


def with_start(batch, doc, pos):
    """The batch with one more word start, at byte `pos` of document `doc` -> a new WordBatch (its expected ids and
    flagged documents are those of the new bitmap)"""
    assert 0 <= pos < batch.lens[doc] and pos not in batch.starts[doc]
    starts = list(batch.starts)
    starts[doc] = sorted(starts[doc] + [pos])
    return WordBatch(batch.lens, starts, batch.doc_spans, batch.lead, batch.tail, batch.junk)


def with_inner_start(batch, doc, token, where):
    """One extra bit strictly inside token `token` of document `doc` (a, b its span) -- where: "a+1", "b-1", or "next":
    the first bit of the bitmap word behind the one that holds a -> (the new batch, the documents that must be flagged)"""
    a, b = batch.doc_spans[doc][token]
    base = int(batch.text_offs[doc])
    pos = {"a+1": a + 1, "b-1": b - 1, "next": ((base + a) // 32 + 1) * 32 - base}[where]
    assert a < pos < b, "no room strictly inside the token"
    out = with_start(batch, doc, pos)
    assert out.flagged == sorted(set(batch.flagged + [doc]))
    return out, out.flagged


# ---- answers ----------------------------------------------------------------------------------------------------------
def span_rows(k, seed):
    """int64[k, 2]: starts and ends both non-decreasing, with ties, overlaps and empty spans among them -- the rule of
    test_closed_form_answers_equal_the_run_qa_loops (tests/test_features_cpu.py), for any k"""
    rnd = random.Random(seed)
    at, spans, last_b = rnd.randrange(0, 4), [], 0
    for _ in range(k):
        a = at + rnd.choice((0, 0, 0, 1))
        b = max(last_b, a + rnd.choice((0, 1, 1, 2, 3)))
        spans.append((a, b))
        last_b = b
        at = b if rnd.random() < 0.8 else a
    return np.array(spans, dtype=np.int64).reshape(-1, 2)


def answers_fast(plan, side, spans, ans):
    """features_ref.answers in closed form: per row two binary searches (np.searchsorted) over the row's a_j and b_j"""
    spans, ans = np.asarray(spans), np.asarray(ans)
    out = np.full((len(plan), 2), -1, dtype=np.int32)
    for r, row in enumerate(np.asarray(plan).tolist()):
        src, k, col = row[5:8] if side == "b" else row[2:5]
        s, e = int(ans[row[0], 0]), int(ans[row[0], 1])
        if s >= e or k <= 0:
            continue
        a, b = spans[src:src + k, 0], spans[src:src + k, 1]
        if a[0] > s or b[-1] < e:
            continue
        out[r] = (col + int(np.searchsorted(a, s, side="right")) - 1, col + int(np.searchsorted(b, e, side="left")))
    return out


def answer_candidates(spans, js):
    """[(s, e)]: for every j of js, s = a_j - 1, a_j, a_j + 1; for each, e = s + 1, b_j, b_last, b_last + 1"""
    last = int(spans[-1, 1])
    out = []
    for j in js:
        a, b = int(spans[j, 0]), int(spans[j, 1])
        for s in (a - 1, a, a + 1):
            out += [(s, s + 1), (s, b), (s, last), (s, last + 1)]
    return out


BIG_J = (0, 1, 62, 63, 64, 65, 4031, 4032, 4095, 4096)


def answer_case(k, side, seed=5, col=3, front=7):
    """One plan whose rows all name the same src / k / col, each its own item -> (plan int64[n, 8], spans int64[front +
    k + 2, 2], ans int64[n, 2]).  The row's spans lie behind `front` others and in front of two more, which differ."""
    own = span_rows(k, seed * 10007 + k)
    if k <= 129:
        js = range(k)
    else:
        rnd = random.Random(seed + k)
        js = sorted({j for j in BIG_J if j < k} | {k - 2, k - 1} | {rnd.randrange(k) for _ in range(200)})
    ans = np.array(answer_candidates(own, js), dtype=np.int64)
    spans = np.concatenate([np.full((front, 2), -3, dtype=np.int64), own, np.full((2, 2), 2 ** 30, dtype=np.int64)])
    plan = np.zeros((len(ans), 8), dtype=np.int64)
    plan[:, 0] = np.arange(len(ans))
    plan[:, 5 if side == "b" else 2] = front
    plan[:, 6 if side == "b" else 3] = k
    plan[:, 7 if side == "b" else 4] = col
    return plan, spans, ans


# ---- word ids: the geometry cases -------------------------------------------------------------------------------------
PER_THREAD = 8  # ids a thread of k_word_ids walks


def doc_of(n, rnd, zeros=True):
    """a document of n tokens: words of one to three tokens of 1..3 bytes, some tokens behind a word's first empty (never
    the document's last: the span at a document's end has a case of its own)"""
    words, left = [], n
    while left:
        w = [rnd.choice((1, 1, 2, 3))] + [rnd.choice((0, 1, 1, 2, 3) if zeros else (1, 2, 3)) for _ in range(min(rnd.randint(0, 2), left - 1))]
        left -= len(w)
        if not left and w[-1] == 0:
            w[-1] = 1
        words.append(w)
    return words


def docs_starting_at(firsts, n_ids, empties, rnd):
    """documents whose first ids are 0 and `firsts` (ascending), n_ids in all, with `empties` empty documents in front of
    each of `firsts` (so at that same id)"""
    edges = [0] + list(firsts) + [n_ids]
    assert all(a < b for a, b in zip(edges, edges[1:]))
    docs = []
    for i, (a, b) in enumerate(zip(edges, edges[1:])):
        if i:
            docs += [[] for _ in range(empties)]
        docs.append(doc_of(b - a, rnd))
    return docs


def edge_firsts(T):
    """the first ids of the case "document starts on edges": the tile's, a wavefront's, and inside one thread's eight"""
    wave = T // 4
    inner = [wave + 40 * PER_THREAD + (PER_THREAD + 1) * r for r in range(PER_THREAD)]  # 8 m + r, r = 0 .. 7
    return sorted([wave - 1, wave, wave + 1] + inner + [T - 1, T, T + 1, 2 * T])


def tile_with_starts(T, n, rnd):
    """exactly n documents start strictly inside tile 1 (T < first id < 2 T); the last of them runs into tile 2"""
    firsts = [T + 5 + i for i in range(n)] + [2 * T + 10]
    return docs_starting_at(firsts, 2 * T + 30, 0, rnd)


def word_cases(T):
    """name -> WordBatch, in the order of the issue's list; T: the ids a workgroup takes (hutk_debug_word_ids_tile)"""
    rnd = random.Random(11)
    cases = {}
    for e in (0, 1, 3):
        cases["edges, %d empty" % e] = word_batch(docs_starting_at(edge_firsts(T), 2 * T + 9, e, rnd))
    cases["3T one-token documents"] = word_batch([[[rnd.choice((1, 2, 3))]] for _ in range(3 * T)])
    cases["3T one-token documents, two empty behind each"] = word_batch(
        [d for _ in range(3 * T) for d in ([[rnd.choice((1, 2, 3))]], [], [])])
    for n in (256, 257, 513):
        cases["%d starts in tile 1" % n] = word_batch(tile_with_starts(T, n, rnd))
    run = [[] for _ in range(T + 3)]
    cases["runs of empties"] = word_batch(run + [doc_of(T, rnd)] + run + [doc_of(300, rnd)] + run[:700] + [doc_of(50, rnd)] + run)
    cases["a long document"] = word_batch([doc_of(5, rnd), doc_of(3 * T + 5, rnd), doc_of(7, rnd)])
    cases["no ids, 4 documents"] = word_batch([[], [], [], []])
    cases["no documents"] = word_batch([])
    for n in (1, T - 1, T, T + 1):
        cases["%d ids" % n] = word_batch(docs_starting_at([n // 2] if n > 1 else [], n, 1, rnd))
    bit_docs = [[[31], [5], [28], [100], [1]]] + [[[1]] * 64 + [[1, 0, 2]]] + [bits_doc(rnd) for _ in range(40)]
    cases["bit positions"] = word_batch(bit_docs)
    cases["bit positions, lead 37, tail 50"] = word_batch(bit_docs, lead=37, tail=50, junk=True)
    cases["empty spans at a document's end"] = word_batch([[[2, 0]], [[1]], [], [[1, 0], [3, 0, 0]], [[4]], [[31, 0]], [[2], [1, 0]]],
                                                          tail=3, junk=True)
    return cases


def bits_doc(rnd):
    """33 bytes (odd: the next document begins at another bit) of words and tokens of mixed lengths"""
    words, left = [], 33
    while left:
        n = min(left, rnd.randint(1, 9))
        cut = rnd.randint(0, n - 1)
        words.append([cut, n - cut] if cut and rnd.random() < 0.5 else [n])
        left -= n
    return words


def mismatch_base():
    """the batch the mismatch cases write their extra word start into: document 1 has a 2-byte token in the middle of a
    word (token 1), document 3 a 40-byte token that crosses a bitmap word (token 1), document 4 an empty span (token 1)
    and a 1-byte token (token 2) in the middle of a word"""
    return word_batch([[[3], [2]], [[1, 2, 1], [4]], [], [[5, 40, 2], [1]], [[2, 0, 1, 3]], [[6]]], lead=3, tail=2, junk=True)


# (where, document, token) of with_inner_start on mismatch_base(), and (name, document, byte) of the starts that must NOT be flagged
MISMATCHES = (("a+1", 1, 1), ("b-1", 3, 1), ("next", 3, 1))
CONTROLS = (("a start at a", 1, 1), ("a start at b", 1, 3), ("an extra bit on an empty span", 4, 2), ("a start at a 1-byte token", 1, 3),
            ("a start at a, mid-word", 4, 3))


def foreign_spans(batch):
    """[(name, id, spans)]: the batch's spans with ONE token's span made that of another text"""
    out = []
    for name, k in (("a = -1", 3), ("b = a - 1", batch.n_ids // 2), ("b = doc_len + 1", batch.n_ids - 2)):
        d = int(np.searchsorted(batch.id_offs, k, side="right")) - 1
        sp = batch.spans.copy()
        if name == "a = -1":
            sp[k, 0] = -1
        elif name == "b = a - 1":
            sp[k, 1] = sp[k, 0] - 1
        else:
            sp[k, 1] = batch.lens[d] + 1
        out.append((name, k, sp))
    return out
