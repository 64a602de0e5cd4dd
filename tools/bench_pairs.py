#!/usr/bin/env python3
"""Pair collation on the GPU (hutoken_amd.collate_pairs / collate_pair_windows, csrc/hutk_collate.hip) against what a
user of encode_packed_device writes without it, on one GPU in one process; the method of tools/bench_collate.py.

C3 (1 M documents) is encoded once with VG through encode_packed_device.  Both sides are views of that one result: side
A are groups of neighbouring documents of its first half, side B groups of its second half (every G-th entry of the
offsets, so B's offsets begin at a non-zero base).  Per configuration three things are timed with device events, 3
warm-up and `--reps` timed repetitions, alternating:

  (a) new    collate_pairs / collate_pair_windows (the latter with its rows call and its read of the number of rows);
  (b) torch  the compositions of torch ops below that give the same tensors (asserted with torch.equal on every output
             before anything is timed); the windows one reads the number of rows once too;
  (c) copy   one torch.Tensor.copy_ that moves as many bytes as (a) reads plus writes (a copy of half that size), the
             bandwidth yardstick.

Configurations, both max_length 512, bos + one separator + eos, int32, right padding:
  longest_first         A and B groups that hold 256 ids on average, so about half of the pairs are cut;
  only_second windows   stride 128, A single documents, B the join of 16 neighbours.
Bytes moved are computed from shapes.  Writes one JSON file (default profiles/pairs_bench.json) with the ratios
new/torch and new/copy and whether the gap to torch lies outside the torch path's spread; no ratio is required.

  python tools/bench_pairs.py [--docs N] [--reps R] [--out FILE] [--head NAME]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_collate import summary, timed_alternating  # noqa: E402

BOS, SEP, EOS = 50256, 50255, 50256


def torch_rows(ids, base_a, base_b, ka, kb, L):
    """Rows [BOS] A' SEP B' [EOS], right padding with 0, int32: (input_ids, attention_mask, token_type_ids, lengths)."""
    import torch
    dev = ids.device
    sl = ka + kb + 3
    col = torch.arange(L, device=dev)[None, :]
    valid = col < sl[:, None]
    end_a = (1 + ka)[:, None]
    top = ids.numel() - 1
    from_a = ids[(base_a[:, None] + col - 1).clamp_(0, top)]
    from_b = ids[(base_b[:, None] + col - 1 - end_a).clamp_(0, top)]
    out = torch.where(valid, torch.where(col < end_a, from_a, from_b), torch.tensor(0, dtype=torch.int32, device=dev))
    out = torch.where(col == end_a, torch.tensor(SEP, dtype=torch.int32, device=dev), out)
    out = torch.where(col == sl[:, None] - 1, torch.tensor(EOS, dtype=torch.int32, device=dev), out)
    out[:, 0] = BOS
    return out, valid.to(torch.uint8), (valid & (col > end_a)).to(torch.uint8), sl.to(torch.int32)


def torch_collate_pairs(ids, offs_a, offs_b, L):
    """longest_first"""
    import torch
    R = L - 3
    la, lb = offs_a[1:] - offs_a[:-1], offs_b[1:] - offs_b[:-1]
    n1, n2 = torch.minimum(la, lb), torch.maximum(la, lb)
    n2 = torch.where(n1 > R, n1, torch.maximum(n1, R - n1))
    over = n1 + n2 > R
    n1 = torch.where(over, R // 2, n1)
    n2 = torch.where(over, R // 2 + R % 2, n2)
    fits, swap = la + lb <= R, la > lb
    ka = torch.where(fits, la, torch.where(swap, n2, n1))
    kb = torch.where(fits, lb, torch.where(swap, n1, n2))
    return torch_rows(ids, offs_a[:-1], offs_b[:-1], ka, kb, L)


def torch_collate_pair_windows(ids, offs_a, offs_b, L, stride):
    """only_second: torch_rows' four and row_map"""
    import torch
    dev = ids.device
    R = L - 3
    n = offs_a.numel() - 1
    la, lb = offs_a[1:] - offs_a[:-1], offs_b[1:] - offs_b[:-1]
    ko = la.clamp(max=R)
    C = R - ko
    step = (C - stride).clamp_(min=1)
    w = torch.where((lb <= C) | (C == 0), 1, 1 + (lb - C + step - 1) // step)
    first = torch.cumsum(w, 0) - w
    n_rows = int(w.sum().item())
    pair = torch.repeat_interleave(torch.arange(n, device=dev), w, output_size=n_rows)
    start = (torch.arange(n_rows, device=dev) - first[pair]) * step[pair]
    kb = torch.minimum(lb[pair] - start, C[pair])
    return torch_rows(ids, offs_a[:-1][pair], offs_b[:-1][pair] + start, ko[pair], kb, L) + (torch.stack([pair, start], dim=1),)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pairs: no GPU; there is nothing to measure without one")
    import hutoken_amd as H
    from hutoken_amd import data, synth
    head = args.head
    if head is None:
        try:
            head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                           stderr=subprocess.DEVNULL).strip()
        except Exception:
            head = "unknown"
    dev = torch.device("cuda", 0)
    vp, sp, kw = data.vocab_files("VG")
    H.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", args.docs)
    st = torch.cuda.Stream(dev)  # a stream of torch's own: the encode is then ordered with everything else here
    results = {"git_head": head, "device": torch.cuda.get_device_name(0), "corpus": "C3", "vocab": "VG",
               "docs": args.docs, "bytes": int(o[-1]), "reps": args.reps, "warmup": 3, "configs": []}
    L, tpl = 512, dict(bos_id=BOS, sep_ids=(SEP,), eos_id=EOS, pad_id=0)
    with torch.cuda.stream(st):
        ids, oo = H.encode_packed_device(torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev))
        n_ids = int(oo[-1].item())
        results["ids"] = n_ids
        half = args.docs // 2
        G = max(1, -(-(L // 2) * args.docs // max(n_ids, 1)))
        n1 = half // G
        a1, b1 = oo[0:n1 * G + 1:G].contiguous(), oo[half:half + n1 * G + 1:G].contiguous()
        n2 = half // 16
        a2, b2 = oo[0:n2 + 1], oo[half:half + n2 * 16 + 1:16].contiguous()
        configs = (
            ("L=512 longest_first bos+sep+eos int32", n1, a1, b1, {"group_a": G, "group_b": G},
             lambda: H.collate_pairs(ids, a1, ids, b1, L, **tpl), lambda: torch_collate_pairs(ids, a1, b1, L)),
            ("L=512 stride=128 only_second windows bos+sep+eos int32", n2, a2, b2, {"group_a": 1, "group_b": 16},
             lambda: H.collate_pair_windows(ids, a2, ids, b2, L, 128, **tpl),
             lambda: torch_collate_pair_windows(ids, a2, b2, L, 128)))
        for name, n, offs_a, offs_b, groups, new, ref in configs:
            got, want = new(), ref()
            torch.cuda.synchronize()
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), name
            n_rows = got[0].shape[0]
            kept = int(got[3].sum().item()) - 3 * n_rows
            windows = len(got) == 5
            del got, want
            # read: the ids of every row, both offsets once per fill workgroup's rows; written: the four outputs.  The
            # windows form reads both offsets twice more (count, write), writes row_offsets, reads it, writes row_map.
            moved = kept * 4 + 2 * (n + 1) * 8 + n_rows * L * 6 + n_rows * 4
            if windows:
                moved += 4 * (n + 1) * 8 + 2 * (n + 1) * 8 + n_rows * 16
            src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            t = timed_alternating({"new": new, "torch": ref, "copy": lambda: dst.copy_(src)}, args.reps)
            r = {"config": name, "pairs": n, "rows": n_rows, "ids_read": kept, "bytes_moved": moved,
                 "pairs_cut": int(((offs_a[1:] - offs_a[:-1]) + (offs_b[1:] - offs_b[:-1]) > L - 3).sum().item()),
                 "new": summary(t["new"]), "torch": summary(t["torch"]), "copy": summary(t["copy"])}
            r.update(groups)
            r["new_GBps"] = moved / r["new"]["median_ms"] / 1e6
            r["copy_GBps"] = moved / r["copy"]["median_ms"] / 1e6
            r["ratio_new_over_torch"] = r["new"]["median_ms"] / r["torch"]["median_ms"]
            r["ratio_new_over_copy"] = r["new"]["median_ms"] / r["copy"]["median_ms"]
            r["gap_to_torch_outside_its_spread"] = abs(1 - r["ratio_new_over_torch"]) > r["torch"]["spread"]
            results["configs"].append(r)
            print(json.dumps(r), flush=True)
            del src, dst
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
