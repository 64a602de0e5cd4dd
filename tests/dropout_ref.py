"""BPE-dropout in plain Python: the rule of hutk_encode_dropout_batch_device (include/hutoken_amd.h) over byte strings.
StringModel: the string-keyed path, {raw key bytes: id}; a pair merges when the concatenation is a key, its rank that
key's id.  RuleModel: a merges file, byte -> id and {(left id, right id): (rank, result id)}.  The words come from
`split(doc) -> ascending word starts` (oracle.split_words, or presplit_ref.word_starts for a preset)."""
import numpy as np

from targets_ref import philox4x32_10, threshold

PURPOSE = 6  # DRAW_BPE_DROPOUT
MAX_WORD_BYTES = 262144  # a longer word ends its document
M32 = 0xFFFFFFFF


class Model:
    def __init__(self, unit, pair, id_of):
        self.unit, self.pair, self.id_of = unit, pair, id_of  # byte -> unit; (left, right) -> (rank, merged) or None; unit -> id


def StringModel(vocab):
    return Model(lambda b: bytes([b]), lambda l, r: (vocab[l + r], l + r) if l + r in vocab else None, lambda tok: vocab.get(tok, -1))


def RuleModel(byte_ids, rules):
    return Model(lambda b: byte_ids[b], lambda l, r: rules.get((l, r)), lambda tok: tok)


def philox_drops(seed, doc, drop_below):
    """-> drops(offsets, t): which of the candidates whose left units begin at these offsets of document `doc` are dropped at step t"""
    def drops(offsets, t):
        x = philox4x32_10((doc & M32, doc >> 32, np.asarray(offsets, dtype=np.uint64) & np.uint64(M32), (t << 4) | PURPOSE),
                          (seed & M32, seed >> 32))[0]
        return [int(v) < drop_below for v in np.atleast_1d(x)]
    return drops


def encode_word(model, word, o0, drops):
    """The ids of one word (bytes) whose first byte is at offset o0 of its document."""
    toks = [(o0 + i, model.unit(b)) for i, b in enumerate(word)]  # (offset of the unit's first byte, the unit)
    hits = [model.pair(toks[k][1], toks[k + 1][1]) for k in range(len(toks) - 1)]  # of the pair (k, k + 1); priced again beside a merge
    t = 0
    while True:
        cands = [(hit[0], k, hit[1]) for k, hit in enumerate(hits) if hit is not None]  # (rank, position in toks, merged)
        if not cands:
            break
        gone = drops([toks[k][0] for _r, k, _m in cands], t)
        alive = [c for c, g in zip(cands, gone) if not g]
        if not alive:
            break
        _rank, k, merged = min(alive, key=lambda c: (c[0], c[1]))  # smallest rank, leftmost on ties
        toks[k:k + 2] = [(toks[k][0], merged)]
        del hits[k]
        for j in (k - 1, k):
            if 0 <= j < len(toks) - 1:
                hits[j] = model.pair(toks[j][1], toks[j + 1][1])
        t += 1
    return [model.id_of(tok) for _o, tok in toks]


def encode_docs(model, docs, split, p, seed, first_doc=0):
    """-> (ids, out_offsets) of the documents (bytes); no word is longer than MAX_WORD_BYTES bytes."""
    ids, offs = [], [0]
    for d, doc in enumerate(docs):
        starts = split(doc) + [len(doc)]
        drops = philox_drops(seed, first_doc + d, threshold(p))
        for a, b in zip(starts[:-1], starts[1:]):
            assert b - a <= MAX_WORD_BYTES
            ids += encode_word(model, doc[a:b], a, drops)
        offs.append(len(ids))
    return ids, offs


def distribution(model, word, p):
    """{tuple of ids: probability} of one word in closed form: at a step with m candidates the k-th best (k from 1) is
    applied with probability p^(k - 1) (1 - p), and the word is finished with probability p^m."""
    out = {}

    def walk(toks, prob):
        cands = sorted((hit[0], k, hit[1]) for k in range(len(toks) - 1) for hit in [model.pair(toks[k], toks[k + 1])] if hit is not None)
        stop = prob * p ** len(cands)
        if stop > 0:
            key = tuple(model.id_of(t) for t in toks)
            out[key] = out.get(key, 0.0) + stop
        for j, (_rank, k, merged) in enumerate(cands):
            if p < 1:
                walk(toks[:k] + [merged] + toks[k + 2:], prob * p ** j * (1 - p))
    walk([model.unit(b) for b in word], 1.0)
    return out
