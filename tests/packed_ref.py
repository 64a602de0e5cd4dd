"""NumPy restatement of packed rows for training (include/hutoken_amd.h, "PACKED CHANNELS" and "PACKED ROWS FOR
TRAINING"), written from the definitions: a packer that moves per-token channels with the ids,
cu_seqlens from segment ids, and the loss labels of packed rows.  tests/test_packed_cpu.py pins it by hand.
Own code; nothing here touches the GPU or the package under test."""
import numpy as np

import collate_ref as R


class Packer(R.Packer):
    """collate_ref.Packer with channels: `channels` is a list of (numpy dtype, per, fill).  Beside the stream S runs one
    stream per channel: the token's record where S holds a document id, the fill where the packer put bos or eos.
    add() and flush() return the parent's dict plus "channels", a list of [rows, L] (per == 2: [rows, L, 2]) arrays."""

    def __init__(self, seq_len, bos_id=None, eos_id=None, pad_id=0, dtype=np.int32, channels=()):
        super().__init__(seq_len, bos_id, eos_id, pad_id, dtype)
        self.channels = [(np.dtype(d), int(per), int(fill)) for d, per, fill in channels]
        self.C = [[] for _ in self.channels]

    def _fill_record(self, c):
        _d, per, fill = self.channels[c]
        return fill if per == 1 else (fill, fill)

    def _channel_rows(self, c, spans):
        """spans: (first row, one past the last stream index) of each row, as the parent's _row takes them"""
        d, per, fill = self.channels[c]
        L = self.L
        out = np.full((len(spans), L) + ((2,) if per == 2 else ()), fill, dtype=d)
        for i, (k, upto) in enumerate(spans):
            if upto > k * L:
                out[i, :upto - k * L] = np.asarray(self.C[c][k * L:upto], dtype=d).reshape((upto - k * L,) + out.shape[2:])
        return out

    def _with_channels(self, rows, spans):
        rows = dict(rows)
        rows["channels"] = [self._channel_rows(c, spans) for c in range(len(self.channels))]
        return rows

    def add(self, ids, offsets, values=()):
        assert len(values) == len(self.channels)
        for i in range(len(offsets) - 1):
            o0, o1 = int(offsets[i]), int(offsets[i + 1])
            for c, v in enumerate(values):
                f = self._fill_record(c)
                rec = [tuple(int(y) for y in x) if self.channels[c][1] == 2 else int(x) for x in v[o0:o1]]
                self.C[c].extend(([f] if self.bos_id is not None else []) + rec + ([f] if self.eos_id is not None else []))
        first = self.done
        rows = super().add(ids, offsets)
        assert all(len(c) == len(self.S) for c in self.C)
        return self._with_channels(rows, [(k, (k + 1) * self.L) for k in range(first, self.done)])

    def flush(self):
        spans = [(self.done, len(self.S))] if self.pending else []
        ch = [self._channel_rows(c, spans) for c in range(len(self.channels))]
        rows = dict(super().flush())
        rows["channels"] = ch
        self.C = [[] for _ in self.channels]
        return rows


def cat(parts):
    """the dicts of several add / flush calls -> one, rows concatenated"""
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("input_ids", "position_ids", "segment_ids")}
    out["channels"] = [np.concatenate([p["channels"][c] for p in parts]) for c in range(len(parts[0]["channels"]))]
    return out


def cu_seqlens(seg, cap):
    """seg int32 [n_rows, L] -> (cu_seqlens int32 [cap + 1], (n_seq, max_seqlen)).  Flat element r * L + c starts a
    sequence when c == 0 or seg[r][c] != seg[r][c - 1]; the first `cap` starts, then n_rows * L in every remaining slot;
    max_seqlen is the largest difference of neighbouring entries."""
    seg = np.asarray(seg, dtype=np.int32)
    n_rows, L = seg.shape
    starts = [r * L + c for r in range(n_rows) for c in range(L) if c == 0 or seg[r, c] != seg[r, c - 1]]
    cu = np.full(cap + 1, n_rows * L, dtype=np.int32)
    cu[:min(cap, len(starts))] = starts[:cap]
    return cu, (len(starts), int(np.diff(cu).max()) if cap and len(starts) else 0)


def cu_seqlens_vec(seg, cap):
    """the same without a Python loop, for the larger shapes (pinned against cu_seqlens by the CPU test)"""
    seg = np.asarray(seg, dtype=np.int32)
    n_rows, L = seg.shape
    start = np.ones(seg.shape, dtype=bool)
    start[:, 1:] = seg[:, 1:] != seg[:, :-1]
    starts = np.flatnonzero(start.reshape(-1))
    cu = np.full(cap + 1, n_rows * L, dtype=np.int32)
    cu[:min(cap, len(starts))] = starts[:cap]
    return cu, (len(starts), int(np.diff(cu).max()) if cap and len(starts) else 0)


def labels(values, seg, shift, ignore):
    """shift False: values where seg != 0, ignore elsewhere.  shift True: labels[r][c] = values[r][c + 1] when c + 1 < L
    and seg[r][c + 1] == seg[r][c] != 0, ignore elsewhere."""
    values, seg = np.asarray(values), np.asarray(seg)
    out = np.full(values.shape, ignore, dtype=values.dtype)
    n_rows, L = values.shape
    for r in range(n_rows):
        for c in range(L):
            if not shift:
                if seg[r, c] != 0:
                    out[r, c] = values[r, c]
            elif c + 1 < L and seg[r, c + 1] == seg[r, c] and seg[r, c] != 0:
                out[r, c] = values[r, c + 1]
    return out


def labels_vec(values, seg, shift, ignore):
    values, seg = np.asarray(values), np.asarray(seg)
    out = np.full(values.shape, ignore, dtype=values.dtype)
    if not shift:
        keep = seg != 0
        out[keep] = values[keep]
    else:
        keep = (seg[:, 1:] == seg[:, :-1]) & (seg[:, :-1] != 0)
        out[:, :-1][keep] = values[:, 1:][keep]
    return out
