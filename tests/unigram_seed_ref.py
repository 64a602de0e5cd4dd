"""The rule of the Unigram seed (include/hutoken_amd.h) restated in plain Python: dictionaries over every
substring of the unique words, integers throughout, no hashing.  The fold is unigram_ref's."""
import collections
import math

import unigram_ref as R


def unique_words(docs, **shape):
    """{folded word (U+2581 as 0x20): occurrences}, in the order of first insertion"""
    words = collections.Counter()
    for d in docs:
        for w in R.words(d, **shape):
            words[w.replace(R.META, b" ")] += 1
    return words


def tables(words, max_piece_length=16):
    """-> (count per character, freq per substring, the set of followers per substring; None is END)"""
    count, freq, followers = collections.Counter(), collections.Counter(), collections.defaultdict(set)
    for w, n_w in words.items():
        for seg in w.split(b"\0"):
            cs = [seg[p:p + ln] for p, ln, _cp in R.chars(seg)]
            for c in cs:
                count[c] += n_w
            for i in range(len(cs)):
                for k in range(2, min(max_piece_length, len(cs) - i) + 1):
                    s = b"".join(cs[i:i + k])
                    freq[s] += 1
                    followers[s].add(cs[i + k] if i + k < len(cs) else None)
    return count, freq, followers


def text(b):
    return ("▁" + b[1:].decode("utf-8", "surrogateescape")) if b[:1] == b" " else b.decode("utf-8", "surrogateescape")


def seed(docs, seed_size=1_000_000, max_piece_length=16, unk_token="<unk>", **shape):
    """-> [(piece, score)] with the unknown line first"""
    count, freq, followers = tables(unique_words(docs, **shape), max_piece_length)
    lines = sorted(((c, s) for s, c in count.items()), reverse=True)
    cands = sorted(((freq[s] * len(R.chars(s)), s) for s in freq if len(followers[s]) >= 2), reverse=True)
    lines += cands[:max(seed_size - 1 - len(lines), 0)]
    total = sum(c for c, _s in lines)
    return [(unk_token, 0.0)] + [(text(s), math.log(c) - math.log(total)) for c, s in lines]
