"""A plain restatement of the decode direction for vocabularies made by the builders of tests/helpers.py: what
hutk_decode_batch must write for a packed batch of ids.  tests/test_decode_cpu.py pins it against the CPU oracle
(which tests/test_oracle_vs_reference.py pins against the reference); the GPU tests compare with it bit for bit.

    byte mode       a document is the concatenation of its tokens' raw bytes, less a prefix at its front
    character mode  the tokens' strings are concatenated, one prefix is taken from the front of the document, then
                    special values go back to their bytes ("▁" -> space, "<0xHH>" of the special file -> that byte)

decode_doc() does exactly that, a document at a time.  decode_packed() does the same for a whole batch with numpy (per
token tables and one gather), so that a batch of 300 k ids costs milliseconds; the two are compared in the CPU test.
The builders' tokens are whole characters and whole special values, so a token's bytes do not depend on its neighbours.
"""
import numpy as np

from hutoken_amd import vocab_files as vf

DOC_ID_OUT_OF_RANGE = 3  # HUTK_DOC_ID_OUT_OF_RANGE
DOC_ID_UNDECODABLE = 4   # HUTK_DOC_ID_UNDECODABLE


def _unspecial(s, values):
    """Character mode, left to right: the longest special value that matches gives its byte, any other character stays."""
    out = bytearray()
    p = 0
    while p < len(s):
        best = None
        for v, b in values:
            if s.startswith(v, p) and (best is None or len(v) > len(best[0])):
                best = (v, b)
        if best:
            out.append(best[1])
            p += len(best[0])
        else:
            out += s[p].encode("utf-8")
            p += 1
    return bytes(out)


class DecodeRef:
    def __init__(self, entries, special, prefix, is_byte):
        """entries [(key bytes, id)] and the special mapping as helpers' builders return them; prefix as given to the
        context (a str or None)."""
        self.n = len(entries)  # ids 0 .. number of vocabulary lines - 1 are in range
        self.is_byte = is_byte
        self.prefix = prefix or ""
        self.values = [(v, b) for b, v in special.items() if v]
        back = {c: b for b, c in vf.bytes_to_unicode().items()}
        self.keys = [None] * self.n  # id -> key string; None: no key has the id, or several have
        count = [0] * self.n
        for key, i in entries:
            if 0 <= i < self.n:
                count[i] += 1
                self.keys[i] = key.decode("utf-8")
        for i in range(self.n):
            if count[i] != 1:
                self.keys[i] = None
        self._visible = back
        # per id: its bytes inside a document and at the front of one
        blob, off, ln, soff, sln = bytearray(), [], [], [], []
        for k in self.keys:
            full = b"" if k is None else self._text(k)
            front = full if k is None or not (self.prefix and k.startswith(self.prefix)) else self._text(k[len(self.prefix):])
            off.append(len(blob)); ln.append(len(full)); blob += full
            soff.append(len(blob)); sln.append(len(front)); blob += front
        self.blob = np.frombuffer(bytes(blob) + b"\0", dtype=np.uint8)
        self.off, self.len = np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int64)
        self.soff, self.slen = np.asarray(soff, dtype=np.int64), np.asarray(sln, dtype=np.int64)
        self.bad = np.asarray([k is None for k in self.keys], dtype=bool)

    def _text(self, s):
        if self.is_byte:
            return bytes(self._visible[c] for c in s)
        return _unspecial(s, self.values)

    def decode_doc(self, ids):
        """One document, the plain way -> (bytes, status)."""
        for i in ids:
            if i < 0 or i >= self.n:
                return b"", DOC_ID_OUT_OF_RANGE
        for i in ids:
            if self.keys[i] is None:
                return b"", DOC_ID_UNDECODABLE
        s = "".join(self.keys[i] for i in ids)
        if self.prefix and s.startswith(self.prefix):
            s = s[len(self.prefix):]
        return self._text(s), 0

    def status(self, ids, id_offsets):
        """int32[n_docs]: 0, or the code of the document's bad id (one kind of bad id per batch)."""
        ids = np.asarray(ids, dtype=np.int64)
        offs = np.asarray(id_offsets, dtype=np.int64)
        in_range = (ids >= 0) & (ids < self.n)
        code = np.where(in_range, 0, DOC_ID_OUT_OF_RANGE)
        code[in_range] = np.where(self.bad[ids[in_range]], DOC_ID_UNDECODABLE, 0)
        st = np.zeros(len(offs) - 1, dtype=np.int32)
        where = np.nonzero(code)[0]
        st[np.searchsorted(offs, where, side="right") - 1] = code[where]
        return st

    def _layout(self, ids, id_offsets):
        ids = np.asarray(ids, dtype=np.int64)
        offs = np.asarray(id_offsets, dtype=np.int64)
        ok = (ids >= 0) & (ids < self.n)
        safe = np.where(ok, ids, 0)
        ok &= ~self.bad[safe]
        first = np.zeros(len(ids), dtype=bool)
        first[offs[:-1][offs[:-1] < offs[1:]]] = True
        ln = np.where(first, self.slen[safe], self.len[safe])
        ln[~ok] = 0
        return ln, np.where(first, self.soff[safe], self.off[safe]), offs

    def lengths(self, ids, id_offsets):
        """bytes that each id of the batch decodes to (a bad id: none)"""
        return self._layout(ids, id_offsets)[0]

    def decode_packed(self, ids, id_offsets):
        """-> (bytes uint8, out_offsets int64[n_docs + 1]).  A bad id contributes no bytes (its document has a status)."""
        ln, src, offs = self._layout(ids, id_offsets)
        n = len(ln)
        pos = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(ln, out=pos[1:])
        take = np.arange(pos[n], dtype=np.int64) + np.repeat(src - pos[:n], ln)
        return self.blob[take], pos[offs]
