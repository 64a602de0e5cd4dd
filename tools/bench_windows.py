#!/usr/bin/env python3
"""Window collation on the GPU (hutoken_amd.collate_windows, csrc/hutk_collate.hip) against what a user of
encode_packed_device writes without it, on one GPU in one process; the method of tools/bench_collate.py.

C3 (1 M documents) is encoded once with VG through encode_packed_device.  Per configuration the documents are joined in
groups of G neighbours (every G-th entry of the offsets), G chosen so that the mean group holds four rows' worth of ids
and most groups exceed max_length; then three things are timed with device events, 3 warm-up and `--reps` timed
repetitions, alternating:

  (a) new    collate_windows(ids, offsets, L, stride, n_ids=n_ids): the rows call, the read of the number of rows, the fill;
  (b) torch  torch_collate_windows below: a straightforward composition of torch ops that gives the same four tensors
             (asserted with torch.equal on every output before anything is timed); it reads the number of rows once too;
  (c) copy   one torch.Tensor.copy_ that moves as many bytes as (a) reads plus writes (a copy of half that size), the
             bandwidth yardstick.

Configurations: max_length 512, stride 128, bos and eos; max_length 2048, stride 0, no bos/eos; int32, right padding.
Bytes moved are computed from shapes.  Writes one JSON file (default profiles/windows_bench.json), and fails when there
is no GPU or when (a) is not faster than (b) by more than (b)'s spread.

  python tools/bench_windows.py [--docs N] [--reps R] [--out FILE] [--head NAME]
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

EOT = 50256


def torch_collate_windows(ids, offsets, n_ids, L, stride, bos_id, eos_id, pad_id):
    """Right padding, int32: (input_ids, attention_mask, lengths, row_map)."""
    import torch
    dev = ids.device
    s = (bos_id is not None) + (eos_id is not None)
    C = L - s
    step = C - stride
    n_docs = offsets.numel() - 1
    lens = offsets[1:] - offsets[:-1]
    w = torch.where(lens <= C, 1, 1 + (lens - C + step - 1) // step)
    first = torch.cumsum(w, 0) - w  # row_offsets[:-1]
    n_rows = int(w.sum().item())
    doc = torch.repeat_interleave(torch.arange(n_docs, device=dev), w, output_size=n_rows)
    start = (torch.arange(n_rows, device=dev) - first[doc]) * step
    sl = torch.clamp(lens[doc] - start, max=C) + s
    col = torch.arange(L, device=dev)[None, :]
    valid = col < sl[:, None]
    idx = (offsets[:-1][doc][:, None] + start[:, None] + col - int(bos_id is not None)).clamp_(0, max(n_ids - 1, 0))
    out = torch.where(valid, ids[idx], torch.tensor(pad_id, dtype=torch.int32, device=dev))
    if eos_id is not None:
        out = torch.where(col == sl[:, None] - 1, torch.tensor(eos_id, dtype=torch.int32, device=dev), out)
    if bos_id is not None:
        out[:, 0] = bos_id
    return out, valid.to(torch.uint8), sl.to(torch.int32), torch.stack([doc, start], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_windows: no GPU; there is nothing to measure without one")
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
    ok = True
    with torch.cuda.stream(st):
        ids, oo = H.encode_packed_device(torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev))
        n_ids = int(oo[-1].item())
        results["ids"] = n_ids
        for L, stride, bos, eos in ((512, 128, EOT, EOT), (2048, 0, None, None)):
            s = (bos is not None) + (eos is not None)
            G = max(1, -(-4 * L * args.docs // max(n_ids, 1)))
            offs = torch.cat([oo[:-1:G], oo[-1:]]).contiguous()
            n_docs = offs.numel() - 1
            lens = offs[1:] - offs[:-1]

            def new():
                return H.collate_windows(ids, offs, L, stride, bos_id=bos, eos_id=eos, pad_id=0, n_ids=n_ids)

            def ref():
                return torch_collate_windows(ids, offs, n_ids, L, stride, bos, eos, 0)

            got, want = new(), ref()
            torch.cuda.synchronize()
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), (L, stride)
            n_rows = got[0].shape[0]
            kept = int(got[2].sum().item()) - s * n_rows
            del got, want
            # read: the ids of every window, offsets twice (count, write) and once per fill workgroup's documents,
            # row_offsets once; written: row_offsets, the four outputs
            moved = kept * 4 + 3 * (n_docs + 1) * 8 + 2 * (n_docs + 1) * 8 + n_rows * L * 5 + n_rows * 4 + n_rows * 16
            half = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            other = torch.empty_like(half)
            t = timed_alternating({"new": new, "torch": ref, "copy": lambda: other.copy_(half)}, args.reps)
            r = {"config": "L=%d stride=%d %s int32" % (L, stride, "bos+eos" if s == 2 else "no bos/eos"),
                 "group": G, "documents": n_docs, "documents_longer_than_a_row": int((lens > L - s).sum().item()),
                 "rows": n_rows, "ids_read": kept, "bytes_moved": moved,
                 "new": summary(t["new"]), "torch": summary(t["torch"]), "copy": summary(t["copy"])}
            r["new_GBps"] = moved / r["new"]["median_ms"] / 1e6
            r["copy_GBps"] = moved / r["copy"]["median_ms"] / 1e6
            r["ratio_new_over_torch"] = r["new"]["median_ms"] / r["torch"]["median_ms"]
            r["ratio_new_over_copy"] = r["new"]["median_ms"] / r["copy"]["median_ms"]
            r["faster_than_torch_beyond_its_spread"] = r["ratio_new_over_torch"] < 1 - r["torch"]["spread"]
            ok &= r["faster_than_torch_beyond_its_spread"]
            results["configs"].append(r)
            print(json.dumps(r), flush=True)
            del half, other
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        sys.exit("bench_windows: the HIP path is not faster than the torch composition in every configuration")


if __name__ == "__main__":
    main()
