"""Unigram training restated in Python and numpy f64 (the rule: include/hutoken_amd.h, "Unigram training"; DESIGN.md section
8n.2): forward-backward, the M-step with its own digamma, the barred best path, the loss, the loop and the finalising.
Words are bytes with their U+2581 spelled out (unigram_ref.words); scores are by seed id, NaN for a dead piece."""
import collections
import functools
import math

import numpy as np

import unigram_ref as R
import unigram_sample_ref as S


def model(pieces, scores, unk_id):
    """The alive pieces as a unigram_ref.Vocab: dead lines and the unknown line's own text are no keys."""
    v = R.Vocab([(p, 0.0 if s != s else s) for p, s in zip(pieces, scores)], unk_id)
    alive = {i for i, s in enumerate(scores) if s == s and i != unk_id}
    v.ids = {p: i for p, i in v.ids.items() if i in alive}
    v.unk_score = min(scores[i] for i in alive) - 10.0
    return v


def corpus_words(docs, **options):
    return [w for d in docs for w in R.words(d, **options)]


def e_step(v, words, n_pieces):
    """-> (expected f64[n_pieces], [sum of Z, words], the largest |Z| of a word, the sum of |Z| over the words)"""
    expected, z_sum, z_top, z_abs = np.zeros(n_pieces), 0.0, 0.0, 0.0
    for w, times in collections.Counter(words).items():  # (every occurrence of a word adds the same)
        lat, bwd, fwd = S.lattice(v, w), {len(w): 0.0}, {0: 0.0}
        for s in sorted(lat, reverse=True):
            bwd[s] = functools.reduce(np.logaddexp, [sc + bwd[e] for e, _i, sc in lat[s]])
        for s in sorted(lat):
            for e, _i, sc in lat[s]:
                fwd[e] = np.logaddexp(fwd.get(e, -np.inf), fwd[s] + sc)
        for s in lat:
            for e, i, sc in lat[s]:
                expected[i] += times * math.exp(fwd[s] + sc + bwd[e] - bwd[0])
        z_sum, z_top, z_abs = z_sum + times * bwd[0], max(z_top, abs(bwd[0])), z_abs + times * abs(bwd[0])
    return expected, [z_sum, float(len(words))], z_top, z_abs


def digamma(x):
    r = 0.0
    while x < 7.0:
        r -= 1.0 / x
        x += 1.0
    x -= 0.5
    xx = 1.0 / x
    xx2 = xx * xx
    xx4 = xx2 * xx2
    return r + math.log(x) + (1.0 / 24.0) * xx2 - (7.0 / 960.0) * xx4 + (31.0 / 8064.0) * xx4 * xx2 - (127.0 / 30720.0) * xx4 * xx4


def m_step(expected, unk_id):
    keep = expected >= 0.5
    keep[unk_id] = False
    of_sum = digamma(float(expected[keep].sum()))
    return np.array([digamma(float(c)) - of_sum if k else np.nan for c, k in zip(expected, keep)])


def best_path(v, w, bar=False):
    """-> (ids with the unknowns fused, score), or (None, None) when nothing reaches the end; bar: without the spanning edge"""
    lat, n, best = S.lattice(v, w), len(w), {0: (0.0, None, None)}
    for s in sorted(lat):
        for e, i, sc in lat[s]:
            if not (bar and s == 0 and e == n) and (e not in best or best[s][0] + sc > best[e][0]):
                best[e] = (best[s][0] + sc, s, i)
    if n not in best:
        return None, None
    ids, e = [], n
    while e:
        _c, e, i = best[e]
        ids.append(i)
    return S.fuse(ids[::-1], v.unk_id), best[n][0]


def alternatives(v, pieces, scores):
    """-> (classes: 0 dead, 1 unconditional, 2 dropped, 3 alternative; {id: ids})"""
    cls, alts = [0] * len(pieces), {}
    for p, i in v.ids.items():
        ids, sc = best_path(v, p, bar=True)
        cls[i] = 1 if ids is None else 2 if sc > scores[i] else 3
        if cls[i] == 3:
            alts[i] = ids
    return cls, alts


def histogram(v, words, n_pieces):
    freq = np.zeros(n_pieces, dtype=np.int64)
    for w, times in collections.Counter(words).items():
        np.add.at(freq, best_path(v, w)[0], times)
    return freq


def losses(freq, cls, alts):
    vsum, out = float(freq.sum()), np.full(len(cls), np.nan)
    for i, c in enumerate(cls):
        f = float(freq[i])
        if c == 1:
            out[i] = np.inf
        elif c == 2 or (c == 3 and f == 0.0):
            out[i] = -np.inf
        elif c == 3:
            alt = sum(math.log(freq[a] + f) - math.log(vsum + f * (len(alts[i]) - 1)) for a in alts[i])
            out[i] = f / vsum * (math.log(f) - math.log(vsum) - alt)
    return out


def kept(loss, desired):
    """-> (the ids a prune keeps, the relative gap of the losses either side of the cut: inf when nothing is cut)"""
    size = max(desired, 3 * int(np.count_nonzero(~np.isnan(loss))) // 4)
    keep = [i for i, x in enumerate(loss) if x == np.inf]
    cand = sorted((i for i, x in enumerate(loss) if np.isfinite(x)), key=lambda i: (-loss[i], i))
    k = max(size - len(keep), 0)
    gap = np.inf if not 0 < k < len(cand) else abs(loss[cand[k - 1]] - loss[cand[k]]) / max(abs(loss[cand[k - 1]]), abs(loss[cand[k]]))
    return sorted(keep + cand[:k]), gap


def _apart(scores, what):
    """Neighbours of a descending list of scores differ by more than 1e-6 relative: the order does not hang on the last bits of a sum"""
    assert all(a - b > 1e-6 * abs(b) for a, b in zip(scores, scores[1:])), "%s: two scores lie within 1e-6 of each other: take another seed" % what


def finalize(pieces, scores, unk_id, vocab_size):
    """-> the lines; like the loop it asserts its own margins: at the cut among the remaining pieces and between neighbouring lines"""
    single = [i for i, p in enumerate(pieces) if len(p) == 1 and i != unk_id]
    low, lines, k = float(np.nanmin(scores)), [], 0
    for i in single:
        if scores[i] != scores[i]:
            k += 1
        lines.append((i, low - 1e-4 * k if scores[i] != scores[i] else float(scores[i])))
    rest = sorted((i for i, s in enumerate(scores) if s == s and i not in set(single)), key=lambda i: (-scores[i], i))
    room = max(vocab_size - 1 - len(lines), 0)
    _apart([float(scores[i]) for i in rest[max(room - 1, 0):room + 1]], "the cut")
    lines = sorted(lines + [(i, float(scores[i])) for i in rest[:room]], key=lambda t: (-t[1], t[0]))
    _apart([s for _i, s in lines], "the lines")
    return [(pieces[unk_id], 0.0)] + [(pieces[i], s) for i, s in lines]


def fit(pieces, scores, unk_id, docs, vocab_size, **options):
    """The loop -> (the finalised lines, the longest word in folded bytes, the largest |Z|); its margins are asserted every round"""
    words, desired, scores = corpus_words(docs, **options), vocab_size * 11 // 10, np.array(scores, dtype=np.float64)
    scores[unk_id] = np.nan
    n_top = max(len(w) - 2 * w.count(R.META) for w in words)
    z_top = 0.0
    while True:
        for _ in range(2):
            expected, _stats, z, _abs = e_step(model(pieces, scores, unk_id), words, len(pieces))
            assert np.abs(expected - 0.5).min() > 1e-6, "a count lies within 1e-6 of 0.5: take another seed"
            scores, z_top = m_step(expected, unk_id), max(z_top, z)
        if np.count_nonzero(~np.isnan(scores)) <= desired:
            return finalize(pieces, scores, unk_id, vocab_size), n_top, z_top
        v = model(pieces, scores, unk_id)
        cls, alts = alternatives(v, pieces, scores)
        keep, gap = kept(losses(histogram(v, words, len(pieces)), cls, alts), desired)
        assert gap > 1e-6, "the losses either side of the cut differ by less than 1e-6: take another seed"
        scores = np.array([s if i in set(keep) else np.nan for i, s in enumerate(scores)])
