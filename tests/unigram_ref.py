"""The Unigram rule restated in pure Python with f64: what the `tokenizers` package computes with
models.Unigram(vocab, unk_id, byte_fallback=False) behind a Metaspace pre-tokenizer, and what hutoken_amd.Unigram must
reproduce id for id.  Documents are bytes (or str, encoded with surrogateescape); a byte that strict UTF-8 rejects is a
character of one byte that no piece matches, which is the project's own definition: `tokenizers` takes only str."""

META = "▁".encode("utf-8")
WHITE_SPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000] + list(range(0x2000, 0x200B)))


def to_bytes(doc):
    return doc.encode("utf-8", "surrogateescape") if isinstance(doc, str) else bytes(doc)


def chars(b):
    """The characters of bytes: [(start, length, code point or None for an ill-formed byte)]"""
    out, p, n = [], 0, len(b)
    while p < n:
        b0 = b[p]
        ln = 1 if b0 < 0x80 else 2 if 0xC2 <= b0 < 0xE0 else 3 if 0xE0 <= b0 < 0xF0 else 4 if 0xF0 <= b0 <= 0xF4 else 0
        cp = None
        if ln and p + ln <= n:
            try:
                cp = ord(b[p:p + ln].decode("utf-8"))
            except UnicodeDecodeError:
                cp = None
        if cp is None:
            ln = 1
        out.append((p, ln, cp))
        p += ln
    return out


def collapse(b):
    out = bytearray()
    for i, c in enumerate(b):
        if c == 0x20 and i > 0 and b[i - 1] == 0x20:
            continue
        out.append(c)
    return bytes(out)


def _split_meta(b):
    """Cut in front of every U+2581 (and at the start)."""
    words, start, p = [], 0, b.find(META, 1)
    while p >= 0:
        words.append(b[start:p])
        start, p = p, b.find(META, p + 1)
    words.append(b[start:])
    return words


def words(doc, prepend_scheme="always", whitespace_split=False, collapse_spaces=False):
    """The words of one document, as bytes with U+2581 spelled out."""
    b = to_bytes(doc)
    if collapse_spaces:
        b = collapse(b)
    if not b:
        return []
    if whitespace_split:
        runs, cur = [], bytearray()
        for p, ln, cp in chars(b):
            if cp in WHITE_SPACE:
                if cur:
                    runs.append(bytes(cur))
                cur = bytearray()
            else:
                cur += b[p:p + ln]
        if cur:
            runs.append(bytes(cur))
        out = []
        for r in runs:
            out += _split_meta(r if r.startswith(META) else META + r)
        return out
    b = b.replace(b" ", META)
    if prepend_scheme != "never" and not b.startswith(META):
        b = META + b
    return _split_meta(b)


class Vocab:
    def __init__(self, vocab, unk_id):
        self.pieces = [(to_bytes(p), float(s)) for p, s in vocab]
        self.unk_id = unk_id
        self.ids = {}
        for i, (p, _s) in enumerate(self.pieces):
            self.ids[p] = i  # (the later id wins)
        self.unk_score = min(s for _p, s in self.pieces) - 10.0
        self.max_len = max(len(p) for p, _s in self.pieces)

    def encode_word(self, w):
        """The ids of one word (bytes): encode_optimized, then the fusing of unknowns."""
        n = len(w)
        grid = chars(w)
        ok = {p for p, _ln, _cp in grid} | {n}
        ill = [0] * (n + 1)  # ill-formed bytes in front of a position
        for p, ln, cp in grid:
            for q in range(p + 1, p + ln + 1):
                ill[q] = ill[p] + (cp is None)
        best = [None] * (n + 1)  # (score, start, id)
        best[0] = (0.0, None, None)
        for s, m, cp in grid:
            here = best[s][0]
            single = False
            if cp is not None:
                for ln in range(1, min(self.max_len, n - s) + 1):
                    e = s + ln
                    if e not in ok:
                        continue
                    i = self.ids.get(w[s:e])
                    if i is None or ill[e] != ill[s]:
                        continue
                    cand = self.pieces[i][1] + here
                    if best[e] is None or cand > best[e][0]:
                        best[e] = (cand, s, i)
                    single = single or ln == m
            if not single:
                cand = self.unk_score + here
                if best[s + m] is None or cand > best[s + m][0]:
                    best[s + m] = (cand, s, self.unk_id)
        ids, e = [], n
        while e > 0:
            _sc, s, i = best[e]
            ids.append(i)
            e = s
        ids.reverse()
        out = []
        for i in ids:
            if i == self.unk_id and out and out[-1] == self.unk_id:
                continue
            out.append(i)
        return out

    def encode(self, doc, **options):
        """-> (ids, word_ids) of one document"""
        ids, wids = [], []
        for k, w in enumerate(words(doc, **options)):
            got = self.encode_word(w)
            ids += got
            wids += [k] * len(got)
        return ids, wids

    def encode_docs(self, docs, **options):
        """-> (ids, offsets, word_ids) flat, as the device calls give them"""
        ids, offs, wids = [], [0], []
        for d in docs:
            a, b = self.encode(d, **options)
            ids += a
            wids += b
            offs.append(len(ids))
        return ids, offs, wids


def folded_size(doc, **options):
    """Bytes of the document's folded text, U+2581 counted as one byte."""
    return sum(len(w) - 2 * w.count(META) for w in words(doc, **options))
