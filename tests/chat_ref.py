"""The chat render's rule (include/hutoken_amd.h, "chat"), restated in plain Python and numpy from its statement, not from
the kernels: turns encoded as one document each -> one sequence per conversation,

    [bos]  prefix[role_t] content_t suffix[role_t]  (for every turn t, in order)  tail

with tail = prefix[gen_role] for a generation prompt, else [eos]; and per token the label, the turn's index inside its
conversation and the index of the content token in the encode call's ids."""
import numpy as np

E_ARG, E_CAPACITY = 4, 7
MAX_ROLES, MAX_PART = 16, 32


class Template:
    """prefix / suffix: one list of ids per role; suffix_loss: per role the leading suffix ids that carry loss (None:
    all); bos / eos: an id or None."""

    def __init__(self, prefix, suffix, suffix_loss=None, bos=None, eos=None):
        assert len(prefix) == len(suffix) and 1 <= len(prefix) <= MAX_ROLES
        self.prefix = [list(p) for p in prefix]
        self.suffix = [list(s) for s in suffix]
        self.suffix_loss = [len(s) for s in self.suffix] if suffix_loss is None else list(suffix_loss)
        assert all(0 <= k <= len(s) for k, s in zip(self.suffix_loss, self.suffix))
        self.bos, self.eos = bos, eos
        self.n_roles = len(prefix)

    def tail(self, gen_role):
        if gen_role >= 0:
            assert self.eos is None
            return self.prefix[gen_role]
        return [] if self.eos is None else [self.eos]

    def fixed(self, gen_role=-1):
        return (self.bos is not None) + len(self.tail(gen_role))

    def bound(self, n_conv, n_turns, n_ids, gen_role=-1):
        return n_ids + n_turns * max(len(p) + len(s) for p, s in zip(self.prefix, self.suffix)) + n_conv * self.fixed(gen_role)


def render(tpl, ids, offsets, roles, conv_offsets, gen_role=-1, loss_roles=0, ignore_index=-100):
    """-> dict(out_ids, out_offsets, labels, turn_ids, source, turn_offsets: numpy arrays; err: 0 or E_ARG).
    A turn with a role outside the template or a length below 0 or above n_ids is reported and left out (rendered
    length 0).  The structure itself (offsets from 0 to n_ids, conv_offsets rising from 0 to n_turns) must hold: the
    rule promises nothing otherwise."""
    ids = [int(v) for v in ids]
    offsets = [int(v) for v in offsets]
    roles = [int(v) for v in roles]
    conv = [int(v) for v in conv_offsets]
    n_turns, n_conv, n_ids = len(offsets) - 1, len(conv) - 1, len(ids)
    assert len(roles) == n_turns and offsets[0] == 0 and offsets[-1] == n_ids
    assert conv[0] == 0 and conv[-1] == n_turns and all(a <= b for a, b in zip(conv, conv[1:]))
    err = 0
    out, lab, tid, src, out_offsets, turn_offsets = [], [], [], [], [0], [0]
    tail = tpl.tail(gen_role)
    for i in range(n_conv):
        if tpl.bos is not None:
            out.append(tpl.bos), lab.append(ignore_index), tid.append(-1), src.append(-1)
        for t in range(conv[i], conv[i + 1]):
            r, n = roles[t], offsets[t + 1] - offsets[t]
            if not 0 <= r < tpl.n_roles or n < 0 or n > n_ids:
                err = E_ARG
                turn_offsets.append(turn_offsets[-1])
                continue
            loss = (loss_roles >> r) & 1
            k = t - conv[i]
            for v in tpl.prefix[r]:
                out.append(v), lab.append(ignore_index), tid.append(k), src.append(-1)
            for j in range(offsets[t], offsets[t + 1]):
                if j >= n_ids:  # (a length that can be, at a place that cannot: reported, the element is undefined)
                    err = E_ARG
                    out.append(0), lab.append(ignore_index), tid.append(k), src.append(-1)
                    continue
                out.append(ids[j]), lab.append(ids[j] if loss else ignore_index), tid.append(k), src.append(j)
            for q, v in enumerate(tpl.suffix[r]):
                out.append(v), lab.append(v if loss and q < tpl.suffix_loss[r] else ignore_index), tid.append(k), src.append(-1)
            turn_offsets.append(turn_offsets[-1] + len(tpl.prefix[r]) + n + len(tpl.suffix[r]))
        for v in tail:
            out.append(v), lab.append(ignore_index), tid.append(-1), src.append(-1)
        out_offsets.append(len(out))
    # the closed form the issue states
    fixed = tpl.fixed(gen_role)
    assert out_offsets == [turn_offsets[conv[i]] + i * fixed for i in range(n_conv + 1)]
    return {"out_ids": np.array(out, dtype=np.int32), "out_offsets": np.array(out_offsets, dtype=np.int64),
            "labels": np.array(lab, dtype=np.int32), "turn_ids": np.array(tid, dtype=np.int32),
            "source": np.array(src, dtype=np.int64), "turn_offsets": np.array(turn_offsets, dtype=np.int64), "err": err}
