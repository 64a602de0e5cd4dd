"""Token spans restated in plain Python and NumPy (include/hutoken_amd.h, hutk_token_spans_device).

A cursor walks the document.  A known id covers the bytes of its own decoding -- what the oracle's decode() gives for the
token alone, prefix-stripped when it is the document's first token -- an id of -1 covers the one item at the cursor: a
byte with is_byte_encoder, otherwise the UTF-8 character whose length the lead byte gives (src/pretokenizer.c:14-28), cut
short at the document's end.  tests/test_spans_cpu.py pins this against the oracle's decode of id prefixes.
"""
import numpy as np

MISMATCH = 5  # HUTK_DOC_SPAN_MISMATCH


def item_len(doc, at, is_byte_encoder):
    """Length of the pretokenizer's item that begins at doc[at] (at < len(doc))."""
    if is_byte_encoder:
        return 1
    b = doc[at]
    n = 1 if b < 0x80 else 2 if b & 0xE0 == 0xC0 else 3 if b & 0xF0 == 0xE0 else 4 if b & 0xF8 == 0xF0 else 1
    return min(n, len(doc) - at)


def item_bounds(doc, is_byte_encoder):
    """Every item boundary of the document, 0 and len(doc) included."""
    out, at = [0], 0
    while at < len(doc):
        at += item_len(doc, at, is_byte_encoder)
        out.append(at)
    return out


def starts_before(doc):
    """c[i] = character starts (bytes b with b & 0xC0 != 0x80) in doc[0:i), i = 0 .. len(doc)."""
    a = np.frombuffer(bytes(doc), dtype=np.uint8)
    c = np.zeros(len(a) + 1, dtype=np.int64)
    np.cumsum((a & 0xC0) != 0x80, out=c[1:])
    return c


def to_chars(doc, byte_spans):
    """Byte spans -> character spans: end = starts in doc[0:end); start of a non-empty span = index of the character that
    holds byte `start`; an empty span is (c, c) with the starts in front of it."""
    c = starts_before(doc)
    return [(int(c[s + 1]) - 1 if e > s else int(c[s]), int(c[e])) for s, e in byte_spans]


class TokenText:
    """Per-token decoding from an oracle (oracle.Oracle): first(id) for a document's first token, rest(id) for any
    other; None when the oracle cannot decode the id on its own."""

    def __init__(self, orc):
        self.orc = orc
        self._first, self._rest = {}, {}

    def first(self, i):
        if i not in self._first:
            out, st = self.orc.decode_bytes([i])
            self._first[i] = out if st == 0 else None
        return self._first[i]

    def rest(self, i):
        if i not in self._rest:
            f = self.first(i)
            out, st = self.orc.decode_bytes([i, i])
            self._rest[i] = out[len(f):] if st == 0 and f is not None else None
        return self._rest[i]


def byte_spans(tt, doc, ids, is_byte_encoder):
    """-> (list of (start, end) in bytes, status): status MISMATCH when some known id's decoding is not what the document
    holds at its span (the spans of such a document are unspecified), else 0."""
    doc = bytes(doc)
    at, out, status = 0, [], 0
    for k, i in enumerate(ids):
        i = int(i)
        if i == -1:
            n = item_len(doc, at, is_byte_encoder) if at < len(doc) else 0
            if n == 0:
                status = MISMATCH
        else:
            text = tt.first(i) if k == 0 else tt.rest(i)
            if text is None:
                text, status = b"", MISMATCH
            n = len(text)
            if doc[at:at + n] != text:
                status = MISMATCH
        end = min(at + n, len(doc))
        out.append((at, end))
        at = end
    return out, status


def spans(tt, doc, ids, is_byte_encoder, unit="byte"):
    sp, status = byte_spans(tt, doc, ids, is_byte_encoder)
    return (to_chars(doc, sp) if unit == "char" else sp), status


def batch(tt, data, offs, ids, oo, is_byte_encoder, unit="byte", dtype=np.int32, docs=None):
    """Packed batch -> (spans [n_ids, 2] of dtype, status int32[n_docs]); docs: only these documents (the others' rows
    stay zero)."""
    raw = bytes(np.asarray(data, dtype=np.uint8))
    n = len(offs) - 1
    out = np.zeros((int(oo[n]), 2), dtype=dtype)
    status = np.zeros(n, dtype=np.int32)
    for d in (range(n) if docs is None else docs):
        a, b = int(oo[d]), int(oo[d + 1])
        sp, status[d] = spans(tt, raw[int(offs[d]):int(offs[d + 1])], ids[a:b], is_byte_encoder, unit)
        if b > a:
            out[a:b] = np.asarray(sp, dtype=np.int64).reshape(-1, 2)
    return out, status
