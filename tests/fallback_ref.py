"""Byte fallback restated in plain Python (include/hutoken_amd.h, the byte-fallback section).

Encode side: the plain ids (the oracle's, or the GPU's plain encode, which the other tests pin to the oracle) and the byte
spans of tests/spans_ref.py give the expanded ids: an id of -1 becomes table[b] for the bytes b of its span.  A document
that spans_ref marks (MISMATCH) keeps its plain ids.

Decode side: a document is decoded token by token.  `tokens(id, first)` gives an ordinary token's bytes -- `first`: it is
at the front of a document or of the run behind a special id, where a prefix comes off -- from tests/decode_ref.py
(from_decode_ref) or from the oracle (from_token_text); an id of the table is its one byte, is never stripped and makes
nothing behind it the front of anything.  tests/test_fallback_cpu.py pins both sides.
"""
import numpy as np

import spans_ref as S

DOC_ID_OUT_OF_RANGE, DOC_ID_UNDECODABLE = 3, 4


def expand_doc(doc, ids, spans, mismatch, table):
    if mismatch:
        return [int(i) for i in ids]
    out = []
    for i, (s, e) in zip(ids, spans):
        if int(i) == -1:
            out.extend(int(table[b]) for b in doc[s:e])
        else:
            out.append(int(i))
    return out


def encode(tt, data, offs, ids, oo, is_byte_encoder, table):
    """Plain ids of a packed batch -> (expanded ids int32, out_offsets int64[n + 1], span status int32[n])."""
    raw = bytes(np.asarray(data, dtype=np.uint8))
    n = len(offs) - 1
    parts, out_oo, status = [], np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    total = 0
    for d in range(n):
        doc = raw[int(offs[d]):int(offs[d + 1])]
        row = ids[int(oo[d]):int(oo[d + 1])]
        sp, status[d] = S.byte_spans(tt, doc, row, is_byte_encoder)
        new = expand_doc(doc, row, sp, status[d] != 0, table)
        parts.extend(new)
        total += len(new)
        out_oo[d + 1] = total
    return np.asarray(parts, dtype=np.int32), out_oo, status


def encode_special(oracle, tt, data, offsets, specials, is_byte_encoder, table):
    """specials_ref.encode with every text piece expanded -> (ids int32, out_offsets int64[n + 1], status int32[n])."""
    import specials_ref as SR
    raw = bytes(np.asarray(data, dtype=np.uint8))
    n = len(offsets) - 1
    parts, oo, st = [], np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    for d in range(n):
        for p in SR.pieces(raw[int(offsets[d]):int(offsets[d + 1])], specials):
            if isinstance(p, bytes):
                ids, status = oracle.encode_bytes(p)
                sp, mism = S.byte_spans(tt, p, ids, is_byte_encoder)
                parts.extend(expand_doc(p, ids, sp, mism != 0, table))
                st[d] = max(st[d], int(status))
            else:
                parts.append(int(p))
        oo[d + 1] = len(parts)
    return np.asarray(parts, dtype=np.int32), oo, st


def from_decode_ref(ref):
    """tokens(id, first) -> (bytes, 0) or (b"", status code), from a decode_ref.DecodeRef"""
    blob = ref.blob.tobytes()

    def tokens(i, first):
        if i < 0 or i >= ref.n:
            return b"", DOC_ID_OUT_OF_RANGE
        if ref.bad[i]:
            return b"", DOC_ID_UNDECODABLE
        a, n = (int(ref.soff[i]), int(ref.slen[i])) if first else (int(ref.off[i]), int(ref.len[i]))
        return blob[a:a + n], 0
    return tokens


def from_token_text(tt, n_lines):
    """... from a spans_ref.TokenText (the oracle's decode of the token alone) of a vocabulary of n_lines lines"""
    def tokens(i, first):
        if i < 0 or i >= n_lines:
            return b"", DOC_ID_OUT_OF_RANGE
        text = tt.first(i) if first else tt.rest(i)
        return (b"", DOC_ID_UNDECODABLE) if text is None else (text, 0)
    return tokens


def decode_doc(tokens, ids, table, specials=None, skip=False):
    """One document -> (bytes, status).  specials: None (the plain decode with fallback) or what was installed, as
    decode_special_ref takes it.  A bad id contributes nothing and gives the status."""
    import decode_special_ref as DSR
    byte_of = {int(t): b for b, t in enumerate(table)}
    text = DSR.strings(specials) if specials else {}
    out, status, first = bytearray(), 0, True
    for i in ids:
        i = int(i)
        if i in byte_of:
            out.append(byte_of[i])
            first = False
        elif i in text:
            if not skip:
                out += text[i]
                first = True  # the run behind a marker is a document of its own
        else:
            piece, code = tokens(i, first)
            out += piece
            status = status or code
            first = False
    return bytes(out), status


def decode_packed(tokens, ids, id_offsets, table, specials=None, skip=False):
    """-> (bytes uint8, out_offsets int64[n + 1], status int32[n])"""
    n = len(id_offsets) - 1
    parts, oo, st = [], np.zeros(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int32)
    total = 0
    for d in range(n):
        piece, st[d] = decode_doc(tokens, ids[int(id_offsets[d]):int(id_offsets[d + 1])], table, specials, skip)
        parts.append(piece)
        total += len(piece)
        oo[d + 1] = total
    return np.frombuffer(b"".join(parts), dtype=np.uint8), oo, st
