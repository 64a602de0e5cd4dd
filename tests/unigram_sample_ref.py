"""Unigram subword regularisation restated in Python f64 (the rule: include/hutoken_amd.h), and every
segmentation of a word by brute force.  A word is bytes with its U+2581 spelled out; the draws count FOLDED bytes (U+2581: one)."""
import itertools
import math

import numpy as np

import targets_ref as T
import unigram_ref as R


def lattice(vocab, w):
    """character start -> [(end, id, score)] by rising end: the matching keys and, where none is the single character, the unknown edge"""
    n, grid = len(w), R.chars(w)
    ok, ill = {p for p, _ln, _cp in grid} | {n}, [0] * (n + 1)  # ill: ill-formed bytes in front of a position
    for p, ln, cp in grid:
        for q in range(p + 1, p + ln + 1):
            ill[q] = ill[p] + (cp is None)
    out = {}
    for s, m, cp in grid:
        ends = [s + ln for ln in range(1, min(vocab.max_len, n - s) + 1)] if cp is not None else []
        c = [(e, vocab.ids[w[s:e]], vocab.pieces[vocab.ids[w[s:e]]][1]) for e in ends if e in ok and w[s:e] in vocab.ids and ill[e] == ill[s]]
        out[s] = c if any(e == s + m for e, _i, _sc in c) else sorted(c + [(s + m, vocab.unk_id, vocab.unk_score)])
    return out


def fuse(ids, unk_id):
    return [i for k, i in enumerate(ids) if not (i == unk_id and k > 0 and ids[k - 1] == unk_id)]


def sample_word(vocab, w, alpha, u):
    """u: the uniforms from the word's first folded byte on -> (ids, the smallest |u - c_k| over the draws, c_k = p_1 + .. + p_k, k < last)"""
    n, lat, beta = len(w), lattice(vocab, w), {len(w): 0.0}
    for s in sorted(lat, reverse=True):
        xs = [alpha * sc + beta[e] for e, _i, sc in lat[s]]
        beta[s] = max(xs) + math.log(sum(math.exp(x - max(xs)) for x in xs))
    ids, gap, s = [], math.inf, 0
    while s < n:
        here = u[s - 2 if s and w.startswith(R.META) else s]
        cums = list(itertools.accumulate(math.exp(alpha * sc + beta[e] - beta[s]) for e, _i, sc in lat[s]))
        gap = min([gap] + [abs(here - c) for c in cums[:-1]])
        s, i, _sc = lat[s][next((k for k, c in enumerate(cums) if here < c), len(cums) - 1)]
        ids.append(i)
    return fuse(ids, vocab.unk_id), gap


def sample_docs(vocab, docs, alpha, seed, first_doc, **options):
    """-> (ids, offsets, word_ids, min_gap) flat, as the device call gives them; min_gap: how far every draw stayed from a boundary"""
    ids, offs, wids, gap = [], [0], [], math.inf
    for d, doc in enumerate(docs):
        x, y, _z, _w = T.draw(seed, first_doc + d, np.arange(R.folded_size(doc, **options), dtype=np.uint64), 5)  # 5: DRAW_UNIGRAM
        u, at = [((a << 21) | (b >> 11)) * 2.0 ** -53 for a, b in zip(x.tolist(), y.tolist())], 0
        for k, w in enumerate(R.words(doc, **options)):
            got, g = sample_word(vocab, w, alpha, u[at:])
            ids, wids, gap = ids + got, wids + [k] * len(got), min(gap, g)
            at += len(w) - 2 * w.count(R.META)
        offs.append(len(ids))
    return ids, offs, wids, gap


def segmentations(vocab, w, alpha):
    """Every path through the word's lattice: [(ids with the unknowns fused, probability)], exp(alpha * the scores' sum) normalised"""
    lat, paths = lattice(vocab, w), []

    def walk(s, ids, total):
        if s == len(w):
            paths.append((tuple(fuse(ids, vocab.unk_id)), math.exp(alpha * total)))
        for e, i, sc in lat.get(s, []):
            walk(e, ids + [i], total + sc)
    walk(0, [], 0.0)
    return [(ids, p / sum(q for _ids, q in paths)) for ids, p in paths]
