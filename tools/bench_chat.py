#!/usr/bin/env python3
"""The chat render on the GPU (hutoken_amd.render_chat_device, csrc/hutk_collate.hip) next to two yardsticks, on one GPU
in one process.

A synthetic batch of chat shape -- `--convs` conversations (default 100 000) of 2 to 12 turns, 5 to 400 ids per turn,
roles in turn, a template of ChatML's size (prefix of 3 ids, suffix of 2 with loss on the first, no bos, no eos) -- is put
on the device once; then three things are timed with device events, warmed up, alternating, `--reps` times each:

  (a) render  render_chat_device: the offsets call (count, scan, write, out_offsets) plus the fill; ids and labels,
              and in a second configuration turn ids and source too;
  (b) packed  SequencePacker.add + flush over the same ids and offsets (seq_len 2048, int32), the layout the fill
              resembles, with its own bytes moved;
  (c) torch   torch_render_chat below: the same render composed from torch ops (repeat_interleave, cumsum, index reads
              and writes), asserted equal to (a) on every output before anything is timed.

Bytes moved follow the traffic model of DESIGN.md section 8i: 4 n_ids in, 4 n_out for the ids and 4 n_out for the labels
out, + 4 n_out for the turn ids and + 8 n_out for the source when asked for (the offsets and roles, 20 bytes per turn, are
counted too).  Writes one JSON file (default profiles/chat_bench.json) and prints one line per configuration.

  python tools/bench_chat.py [--convs N] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

IGNORE = -100
PREFIX = {"system": [50257, 9, 198], "user": [50257, 10, 198], "assistant": [50257, 11, 198], "tool": [50257, 12, 198]}
SUFFIX = [50258, 198]


def synthetic_batch(n_conv, seed=0):
    """-> ids int32, offsets int64[n_turns + 1], roles int32[n_turns], conv_offsets int64[n_conv + 1] (numpy)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    turns = rng.integers(2, 13, n_conv)
    conv = np.zeros(n_conv + 1, dtype=np.int64)
    np.cumsum(turns, out=conv[1:])
    n_turns = int(conv[-1])
    lens = rng.integers(5, 401, n_turns)
    offsets = np.zeros(n_turns + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    k = np.arange(n_turns) - np.repeat(conv[:-1], turns)  # the turn's index inside its conversation
    roles = np.where(k == 0, 0, 1 + (k - 1) % 2).astype(np.int32)  # system, then user and assistant in turn
    ids = rng.integers(0, 50257, int(offsets[-1]), dtype=np.int32)
    return ids, offsets, roles, conv


def torch_render_chat(ids, offsets, roles, conv, n_ids, pre, suf, sloss, loss_bits):
    """Without bos, eos and generation prompt (ChatML): (out_ids, out_offsets, labels, turn_ids, source)."""
    import torch
    dev = ids.device
    n_t = offsets[1:] - offsets[:-1]
    pl, sl = pre.shape[1], suf.shape[1]
    lens = n_t + (pl + sl)
    T = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=T[1:])
    n_out = int(T[-1].item())
    p = torch.arange(n_out, device=dev)
    t = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), lens, output_size=n_out)
    u = p - T[t]
    role = roles[t].long()
    nt = n_t[t]
    is_pre, is_suf = u < pl, u >= pl + nt
    src = offsets[t] + u - pl
    v = u - pl - nt
    out = torch.where(is_pre, pre[role, u.clamp(max=pl - 1)],
                      torch.where(is_suf, suf[role, v.clamp(0, sl - 1)], ids[src.clamp(0, max(n_ids - 1, 0))]))
    carries = ((loss_bits >> role) & 1).bool() & ~is_pre & (~is_suf | (v < sloss[role]))
    labels = torch.where(carries, out, torch.tensor(IGNORE, dtype=torch.int32, device=dev))
    conv_of_turn = torch.repeat_interleave(torch.arange(conv.numel() - 1, device=dev), conv[1:] - conv[:-1], output_size=lens.numel())
    turn_ids = (t - conv[conv_of_turn[t]]).to(torch.int32)
    source = torch.where(is_pre | is_suf, torch.tensor(-1, dtype=torch.int64, device=dev), src)
    return out, T[conv], labels, turn_ids, source


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--convs", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chat_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_chat: no GPU; there is nothing to measure without one")
    import hutoken_amd as H
    from bench_collate import summary, timed_alternating
    dev = torch.device("cuda", 0)
    template = H.ChatTemplate({r: (p, SUFFIX, 1) for r, p in PREFIX.items()})
    ids, offsets, roles, conv = (torch.from_numpy(a).to(dev) for a in synthetic_batch(args.convs))
    n_ids, n_turns, n_conv = ids.numel(), roles.numel(), conv.numel() - 1
    pre = torch.tensor(list(PREFIX.values()), dtype=torch.int32, device=dev)
    suf = torch.tensor([SUFFIX] * len(PREFIX), dtype=torch.int32, device=dev)
    sloss = torch.ones(len(PREFIX), dtype=torch.int64, device=dev)
    loss_bits = torch.tensor(1 << template.role_index("assistant"), dtype=torch.int64, device=dev)
    results = {"device": torch.cuda.get_device_name(0), "conversations": n_conv, "turns": n_turns, "ids": n_ids,
               "reps": args.reps, "configs": []}
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        def render(extra):
            return H.render_chat_device(ids, offsets, conv, roles, template, n_ids=n_ids, return_turn_ids=extra, return_source=extra)

        want = torch_render_chat(ids, offsets, roles, conv, n_ids, pre, suf, sloss, loss_bits)
        got = render(True)
        n_out = int(got[1][-1].item())
        results["rendered_ids"] = n_out
        assert torch.equal(got[1], want[1])
        for g, w in zip((got[0], got[2], got[3], got[4]), (want[0], want[2], want[3], want[4])):
            assert g.dtype == w.dtype and torch.equal(g[:n_out], w), "the torch composition and the render differ"
        del got, want
        structure = n_turns * 20 + n_conv * 16
        L = 2048
        packer = H.SequencePacker(L)

        def packed():
            rows = packer.add(ids, offsets, n_ids=n_ids)
            packer.flush()  # every repetition packs the same stream from its start
            return rows

        packed_moved = n_ids * 4 + (n_turns + 1) * 8 + (n_ids // L + 1) * L * 12
        for label, extra, per_out in (("render: ids + labels", False, 8), ("render: ids + labels + turn ids + source", True, 20)):
            moved = n_ids * 4 + n_out * per_out + structure
            fns = {"render": lambda extra=extra: render(extra), "packed": packed}
            if not extra:
                fns["torch"] = lambda: torch_render_chat(ids, offsets, roles, conv, n_ids, pre, suf, sloss, loss_bits)
            t = timed_alternating(fns, args.reps)
            r = {"config": label, "bytes_moved": moved, "render": summary(t["render"]), "packed": summary(t["packed"]),
                 "packed_bytes_moved": packed_moved}
            r["render_GBps"] = moved / r["render"]["median_ms"] / 1e6
            r["packed_GBps"] = packed_moved / r["packed"]["median_ms"] / 1e6
            if "torch" in t:
                r["torch"] = summary(t["torch"])
                r["ratio_render_over_torch"] = r["render"]["median_ms"] / r["torch"]["median_ms"]
            results["configs"].append(r)
            print(json.dumps(r), flush=True)
        packer.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
