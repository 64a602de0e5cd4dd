"""A small pure-Python restatement of the trainer's semantics (tools/train_vocab.cpp, "bytes" mode), for the tests.

  words      oracle.split_words per document (the reference's splitter), counted over all documents
  symbols    bytes 0..255; merge k creates 256 + k
  count      pair (a, b): sum over unique words of count x adjacent (a, b) positions (overlaps count)
  select     highest count, ties to the smaller (a << 32 | b); stop after n_merges or when no count >= 1
  apply      left to right, non-overlapping

Incremental like the C++ trainer: only the words holding the merged pair are rewritten, and the pair counts change by
the difference of those words' old and new pairs; the selection is a heap with lazy deletion."""
import heapq
from collections import Counter, defaultdict


def word_counts(docs, counts=None):
    """docs: iterable of bytes (one document each) -> Counter of word bytes."""
    from oracle import oracle as O
    counts = Counter() if counts is None else counts
    for d in docs:
        if not d:
            continue
        st = O.split_words(d)
        for i, a in enumerate(st):
            b = st[i + 1] if i + 1 < len(st) else len(d)
            counts[d[a:b]] += 1
    return counts


def train_words(counts, n_merges):
    """counts: {word bytes: count} -> (pairs [(a, b)], pair counts [int])."""
    words = [list(w) for w in counts]
    wc = [counts[w] for w in counts]
    pc = defaultdict(int)
    where = defaultdict(set)
    for i, s in enumerate(words):
        for j in range(len(s) - 1):
            pc[(s[j], s[j + 1])] += wc[i]
            where[(s[j], s[j + 1])].add(i)
    heap = [(-c, p) for p, c in pc.items()]  # tuples (a, b) order like the key a << 32 | b
    heapq.heapify(heap)
    pairs, cnts = [], []
    for k in range(n_merges):
        best = None
        while heap:
            c, p = heapq.heappop(heap)
            if pc.get(p, 0) == -c and -c > 0:
                best = (p, -c)
                break
        if best is None:
            break
        (a, b), c = best
        n = 256 + k
        pairs.append((a, b))
        cnts.append(c)
        touched = set()
        for i in sorted(where.pop((a, b), ())):
            s = words[i]
            ns, j = [], 0
            while j < len(s):
                if j + 1 < len(s) and s[j] == a and s[j + 1] == b:
                    ns.append(n)
                    j += 2
                else:
                    ns.append(s[j])
                    j += 1
            if len(ns) == len(s):
                continue
            for j in range(len(s) - 1):
                pc[(s[j], s[j + 1])] -= wc[i]
                touched.add((s[j], s[j + 1]))
            for j in range(len(ns) - 1):
                pc[(ns[j], ns[j + 1])] += wc[i]
                where[(ns[j], ns[j + 1])].add(i)
                touched.add((ns[j], ns[j + 1]))
            words[i] = ns
        for p in touched:
            if pc[p] > 0:
                heapq.heappush(heap, (-pc[p], p))
            else:
                del pc[p]
    return pairs, cnts


def train(docs, n_merges):
    return train_words(word_counts(docs), n_merges)
