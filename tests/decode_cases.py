"""Batches of ids for the decode direction at the sizes where its tile kernel changes path (hutk_decode.hip: tiles of
TILE ids; a tile's text staged in LDS up to STAGE bytes; 16-bit positions up to 65535 bytes of tile text).  Plain
builders without a GPU: tests/test_decode_cpu.py checks a sample of them against the oracle, and
tests/test_gpu_decode_edges.py runs all of them.  Every builder returns (ids int32, id_offsets int64)."""
import random

import numpy as np

import helpers as H
from decode_ref import DecodeRef

TILE = 2048
STAGE = 24576  # DEC_LDS_BYTES


class Vocab:
    """A builder's vocabulary with what a test needs to pick tokens: id by token, ids by decoded length."""

    def __init__(self, kind, seed=1, prefix="default"):
        if kind == "byte":
            self.entries, self.special, self.tokens = H.long_token_byte_vocab(seed)
            self.is_byte, self.prefix = True, None if prefix == "default" else prefix
            self.n_base = len(self.tokens) - 4 * len(H.LONG_BYTE_RUNS)
        else:
            self.entries, self.special, self.tokens = H.long_token_char_vocab(seed)
            self.n_base = len(self.tokens) - 4 * len(H.LONG_CHAR_RUNS)  # (lower when a run existed already)
            for tok in ["▁▁▁"] + ["etaoinsh"[:k] for k in range(2, 9)]:  # decoded lengths 0 .. 8 with the prefix alone
                if tok not in self.tokens:
                    self.entries.append((tok.encode("utf-8"), len(self.tokens)))
                    self.tokens.append(tok)
            self.is_byte, self.prefix = False, "▁"
        self.kind = kind
        self.ref = DecodeRef(self.entries, self.special, self.prefix, self.is_byte)
        self.id = {t: i for i, t in enumerate(self.tokens)}

    def write(self, tmpdir, name):
        return H.write_vocab(tmpdir, name, self.entries, self.special)

    def run(self, ch, k):
        """id of the run token of k times `ch` (bytes in byte mode, str in character mode)"""
        return self.id[ch * k]


def pack(docs):
    offs = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=offs[1:])
    flat = np.asarray([t for d in docs for t in d], dtype=np.int32)
    return flat, offs


def cut(ids, cuts):
    """ids as documents that end at the given positions (repeats = empty documents) and at the end"""
    n = len(ids)
    c = sorted(x for x in cuts if 0 <= x <= n)
    return np.asarray(ids, dtype=np.int32), np.asarray([0] + c + [n], dtype=np.int64)


def cut_random(ids, rng, lo=0, hi=3):
    """documents of lo .. hi tokens"""
    n, cuts, p = len(ids), [], 0
    while p < n:
        p = min(n, p + rng.randint(lo, hi))
        cuts.append(p)
    return cut(ids, cuts[:-1] if cuts and cuts[-1] == n else cuts)


def ordinary(v, rng, n):
    """n ids of the small tokens the random builders make (a staged tile)"""
    return [rng.randrange(v.n_base) for _ in range(n)]


def exact_tile(lens, total, n=TILE):
    """n lengths from the three consecutive values `lens` (lo, lo + 1, lo + 2) that add up to `total`, the odd ones out
    spread over the tile rather than at its end"""
    lo, mid, hi = lens
    out = [mid] * n
    d = total - mid * n
    assert abs(d) <= n
    step = n // (abs(d) + 1) if d else n
    for j in range(abs(d)):
        out[(j + 1) * step - 1] = hi if d > 0 else lo
    assert sum(out) == total
    return out


def tile_total_cases(v, seed=5):
    """Byte mode: a tile of 2048 run tokens whose text is 65535, 65536, 65537 and 614400 bytes, and one of 65567 bytes
    whose last token is the first to have 65536 bytes in front of it; as one-token documents and as documents of
    0 .. 3 tokens, each with an ordinary tile behind it.  -> [(name, ids, offsets)]"""
    rng = random.Random(seed)
    kinds = {31: [v.run(b"-", 31), v.run(b" ", 31), v.id[(b"ab" * 31)[:31]]],
             32: [v.run(b"-", 32), v.run(b" ", 32), v.id[(b"ab" * 32)[:32]], v.run("é".encode(), 16)],
             33: [v.run(b"-", 33), v.run(b" ", 33), v.id[(b"ab" * 33)[:33]]]}
    out = []
    for total in (65535, 65536, 65537, 65567, 300 * TILE):
        if total == 300 * TILE:
            head = [v.run(b"-", 300), v.run(b" ", 300), v.id[(b"ab" * 300)[:300]]]
            head = [head[j % 3] for j in range(TILE)]
        else:
            lens = exact_tile((31, 32, 33), 65536, TILE - 1) + [31] if total == 65567 else exact_tile((31, 32, 33), total)
            head = [kinds[n][j % len(kinds[n])] for j, n in enumerate(lens)]
        tail = ordinary(v, rng, 700)
        ids = head + tail
        out.append(("total%d_one_token_docs" % total, *cut(ids, list(range(1, TILE + 1)) + [TILE + 300])))
        out.append(("total%d_docs_0_to_3" % total, *cut_random(ids, rng)))
    return out


def staging_cases(v, seed=6):
    """Character mode: tiles of exactly 24575, 24576 and 24577 bytes from the 11, 12 and 13 byte "a" runs (the last one
    is not staged), and an unstaged tile of inline and blob tokens between two staged ones of odd length."""
    rng = random.Random(seed)
    a = {n: v.run("a", n) for n in (11, 12, 13)}
    out = []
    for total in (STAGE - 1, STAGE, STAGE + 1):
        ids = ordinary(v, rng, 5) + [a[n] for n in exact_tile((11, 12, 13), total)]
        ids = ids[5:] + ids[:5] + ordinary(v, rng, 300)  # the exact tile first, then a partial one
        out.append(("stage%d" % total, *cut_random(ids, rng, 0, 40)))
    long_ids = [v.run("a", k) for k in (20, 40, 64, 100)] + [v.run("漢", k) for k in (5, 13, 40)] + [v.run("▁", 21)]
    while True:  # (seeded: the same batch every time) until the tiles meet at odd byte addresses
        mixed = [rng.choice(long_ids) if rng.random() < 0.3 else rng.randrange(v.n_base) for _ in range(TILE)]
        ids = ordinary(v, rng, TILE) + mixed + ordinary(v, rng, TILE + 77)
        ids, offs = cut_random(ids, rng, 0, 90)
        offs = np.unique(np.concatenate([offs, [TILE, 2 * TILE]]))  # documents end with the tiles: out_offsets there
        oo = v.ref.decode_packed(ids, offs)[1]
        a, b = (int(oo[np.searchsorted(offs, x)]) for x in (TILE, 2 * TILE))
        if a % 2 and b % 2 and a <= STAGE and b - a > STAGE:
            break
    out.append(("staged_unstaged_staged", ids, offs))
    return out


def inline_cases(v, seed=7):
    """Every decoded length 0 .. 8 next to every other, at every byte alignment: documents that walk through the
    lengths from every starting point, some of them with the prefix alone in front (character mode: length 0)."""
    rng = random.Random(seed)
    if v.kind == "char":
        by_len = {k: v.id["etaoinsh"[:k]] for k in range(1, 9)}
        zero = v.id["▁"]
    else:
        by_len = {}
        for i in range(v.n_base):
            by_len.setdefault(len(v.tokens[i]), i)
        assert all(k in by_len for k in range(1, 9))
        zero = None
    docs = []
    for start in range(1, 9):
        for stride in (1, 3, 5, 7):
            walk = [by_len[(start + j * stride - 1) % 8 + 1] for j in range(rng.randint(8, 30))]
            docs.append(([zero] if zero is not None and rng.random() < 0.5 else []) + walk)
    docs += [[by_len[7], by_len[8]] * 9, [by_len[8], by_len[7]] * 9, [by_len[7]] * 5 + [by_len[8]] * 5]
    docs = docs * 12  # several tiles, so the same walks meet other alignments
    rng.shuffle(docs)
    return [("inline_lengths", *pack(docs))]


SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 4096, 64 * 2048, 64 * 2048 + 1, 65 * 2048 + 1, 129 * 2048 + 5]


def stream(v, n, seed):
    """n ids, nine in ten of them ordinary, the others long run tokens (so some tiles are not staged)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, v.n_base, n)
    long_ = rng.integers(v.n_base, len(v.tokens), n)
    return np.where(rng.random(n) < 0.1, long_, ids).astype(np.int32)


def size_cases(v, n, seed=8):
    """n ids as one document; cut one token before, at and one token after every tile boundary; with runs of 1, 2 and
    300 empty documents at the front, exactly on a tile boundary and at the end."""
    ids = stream(v, n, seed + n)
    out = [("n%d_one_doc" % n, *cut(ids, []))]
    bounds = [t * TILE + d for t in range(1, n // TILE + 2) for d in (-1, 0, 1)]
    out.append(("n%d_cut_at_tiles" % n, *cut(ids, [b for b in bounds if 0 < b < n])))
    mid = (n // TILE // 2 + 1) * TILE if n > TILE else min(n, TILE)  # a tile boundary inside (or the end)
    for run in (1, 2, 300):
        out.append(("n%d_empty%d_front" % (n, run), *cut(ids, [0] * run + [n // 2])))
        out.append(("n%d_empty%d_on_tile" % (n, run), *cut(ids, [min(mid, n)] * (run + 1))))
        out.append(("n%d_empty%d_end" % (n, run), *cut(ids, [n // 3] + [n] * run)))
    return out


def one_id_docs(v, seed=9):
    ids = stream(v, TILE, seed)
    return [("2048_one_id_docs", *cut(ids, list(range(1, TILE)))),
            ("only_empty_docs", np.zeros(0, dtype=np.int32), np.zeros(301, dtype=np.int64))]


def first_token_kinds(v):
    """ids to put at the front of a document: the prefix alone, three prefixes, a 100-character token that starts with
    the prefix (its stripped form lives in the blob), a 100-character token that does not"""
    if v.kind == "char":
        return [v.id["▁"], v.id["▁▁▁"], v.id["▁" + "e" * 100], v.run("a", 100)]
    return [v.id[b" "], v.run(b" ", 32), v.run(b" ", 100), v.run(b"-", 100)]  # (byte mode: no run of three)


def prefix_cases(v, seed=10):
    """Documents whose first token sits on every index mod 32 and on a tile's first and last slot, the first token of
    each kind; the same ids elsewhere in the documents."""
    rng = random.Random(seed)
    kinds = first_token_kinds(v)
    starts = sorted(set(range(0, 3 * TILE, 33)) | {TILE - 1, TILE, 2 * TILE - 1, 2 * TILE})
    n = starts[-1] + 20
    out = []
    for which in range(len(kinds) + 1):
        ids = [rng.choice(kinds) if rng.random() < 0.2 else rng.randrange(v.n_base) for _ in range(n)]
        for j, s in enumerate(starts):
            ids[s] = kinds[which] if which < len(kinds) else kinds[j % len(kinds)]
        out.append(("first_token_kind%d" % which, *cut(ids, starts[1:])))
    return out


def shipped_vocab_ref(files):
    """the DecodeRef of a shipped vocabulary from what hutoken_amd.data.vocab_files returns"""
    from hutoken_amd import vocab_files as vf
    vp, _sp, kw = files
    ents = []
    with open(vp, "r", encoding="ascii") as f:
        for line in f:
            key, _eq, idx = line.partition(" == ")
            ents.append((bytes.fromhex(key.replace("0x", "")), int(idx)))
    return DecodeRef(ents, vf.gpt2_special_mapping(), kw["prefix"], kw["is_byte_encoder"])


def shipped_vocab_case(ref, seed=4):
    """Ids of a shipped vocabulary (`ref` its DecodeRef) in documents of 0 .. 60 tokens: a tile that is half ordinary
    ids and half tokens of 13 bytes and more, three tiles of such tokens alone (at least 13 bytes each less one
    stripped byte per document: not staged), then ordinary ids (about 6 bytes each: staged)."""
    long_ids = np.nonzero((ref.len >= 13) & ~ref.bad)[0]
    assert len(long_ids) >= 1000
    rng = np.random.default_rng(seed)
    ids = np.concatenate([rng.integers(0, ref.n - 1, 1000), rng.choice(long_ids, 3 * TILE + 1048),
                          rng.integers(0, ref.n - 1, 3000)]).astype(np.int32)
    return cut_random(ids, random.Random(seed), 0, 60)
