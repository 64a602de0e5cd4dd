#!/usr/bin/env python3
"""Collation on the GPU (hutoken_amd.SequencePacker / collate_padded, csrc/hutk_collate.hip) against what a user of
encode_packed_device does today, on one GPU in one process.

C3 (1 M documents) is encoded once with VG through encode_packed_device; then, per configuration, three things are timed
with device events, warmed up, alternating, `--reps` times each:

  (a) new    the HIP path;
  (b) torch  torch_collate_packed / torch_collate_padded below: a straightforward composition of torch ops that gives
             the same tensors (asserted with torch.equal on every output before anything is timed);
  (c) copy   one torch.Tensor.copy_ that moves as many bytes as (a) reads plus writes (a copy of half that size: it
             reads and writes each byte), the bandwidth yardstick.

Configurations: packed seq_len 2048 and 8192 with an end-of-text id, int32 and int64; padded max_length 256, right
truncation, right padding, bos and eos, int32.  Bytes moved are computed from shapes.  Also timed: the encode step of
the same batch, next to the packed-2048 collation.  Writes one JSON file (default profiles/collate_bench.json) and
fails when there is no GPU or when (a) is not faster than (b) by more than (b)'s spread.

  python tools/bench_collate.py [--docs N] [--reps R] [--out FILE] [--head NAME]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EOT = 50256


def torch_collate_packed(ids, offsets, n_ids, L, eos_id, dtype):
    """The complete rows of all documents, each followed by eos_id: (input_ids, position_ids, segment_ids)."""
    import torch
    dev = ids.device
    n_docs = offsets.numel() - 1
    lens = offsets[1:] - offsets[:-1] + 1
    b = torch.cumsum(lens, 0) - lens  # where each sequence starts
    T = n_ids + n_docs
    p = torch.arange(T, device=dev)
    j = torch.repeat_interleave(torch.arange(n_docs, device=dev), lens, output_size=T)
    q = p - b[j]
    src = (offsets[:-1][j] + q).clamp_(max=max(n_ids - 1, 0))
    S = torch.where(q == lens[j] - 1, torch.tensor(eos_id, dtype=torch.int32, device=dev), ids[src])
    row_start = p // L * L
    pos = (p - torch.maximum(b[j], row_start)).to(torch.int32)
    f = torch.zeros(T, dtype=torch.int32, device=dev)
    f[b] = 1
    f[::L] = 0
    c = torch.cumsum(f, 0)
    seg = (1 + c - c[row_start]).to(torch.int32)
    rows = T // L
    return (S[:rows * L].view(rows, L).to(dtype), pos[:rows * L].view(rows, L), seg[:rows * L].view(rows, L))


def torch_collate_padded(ids, offsets, n_ids, L, bos_id, eos_id, pad_id, dtype):
    """Right truncation, right padding, bos and eos: (input_ids, attention_mask, lengths)."""
    import torch
    dev = ids.device
    n = (offsets[1:] - offsets[:-1]).clamp_(max=L - 2)
    sl = n + 2
    col = torch.arange(L, device=dev)[None, :]
    valid = col < sl[:, None]
    idx = (offsets[:-1, None] + col - 1).clamp_(0, max(n_ids - 1, 0))
    out = torch.where(valid, ids[idx], torch.tensor(pad_id, dtype=torch.int32, device=dev))
    out = torch.where(col == sl[:, None] - 1, torch.tensor(eos_id, dtype=torch.int32, device=dev), out)
    out[:, 0] = bos_id
    return out.to(dtype), valid.to(torch.uint8), sl.to(torch.int32)


def timed_alternating(fns, reps, warmup=3):
    """fns: {name: callable}; -> {name: [ms] * reps}, the callables run in turn within every repetition."""
    import torch
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return times


def summary(ms):
    s = sorted(ms)
    med = s[len(s) // 2]
    return {"median_ms": med, "min_ms": s[0], "max_ms": s[-1], "spread": (s[-1] - s[0]) / med, "reps": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collate_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_collate: no GPU; there is nothing to measure without one")
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
               "docs": args.docs, "bytes": int(o[-1]), "reps": args.reps, "configs": []}
    ok = True
    with torch.cuda.stream(st):
        d_bytes, d_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
        ids, oo = H.encode_packed_device(d_bytes, d_offs)
        n_docs = oo.numel() - 1
        n_ids = int(oo[-1].item())
        results["ids"] = n_ids
        enc = timed_alternating({"encode": lambda: H.encode_packed_device(d_bytes, d_offs, check=False)}, args.reps)
        results["encode_step"] = summary(enc["encode"])
        read_common = n_ids * 4 + (n_docs + 1) * 8

        def one(label, new, ref, moved):
            got, want = new(), ref()
            torch.cuda.synchronize()
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), label
            del got, want
            half = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            other = torch.empty_like(half)
            t = timed_alternating({"new": new, "torch": ref, "copy": lambda: other.copy_(half)}, args.reps)
            r = {"config": label, "bytes_moved": moved, "new": summary(t["new"]), "torch": summary(t["torch"]),
                 "copy": summary(t["copy"])}
            r["new_GBps"] = moved / r["new"]["median_ms"] / 1e6
            r["copy_GBps"] = moved / r["copy"]["median_ms"] / 1e6
            r["ratio_new_over_torch"] = r["new"]["median_ms"] / r["torch"]["median_ms"]
            r["ratio_new_over_copy"] = r["new"]["median_ms"] / r["copy"]["median_ms"]
            r["faster_than_torch_beyond_its_spread"] = r["ratio_new_over_torch"] < 1 - r["torch"]["spread"]
            results["configs"].append(r)
            print(json.dumps(r), flush=True)
            return r["faster_than_torch_beyond_its_spread"]

        for L in (2048, 8192):
            for dtype in (torch.int32, torch.int64):
                packer = H.SequencePacker(L, eos_id=EOT, dtype=dtype)

                def new(packer=packer):
                    rows = packer.add(ids, oo, n_ids=n_ids)
                    packer.flush()  # every repetition packs the same stream from its start
                    return rows["input_ids"], rows["position_ids"], rows["segment_ids"]

                rows = (n_ids + n_docs) // L
                moved = read_common + rows * L * (dtype.itemsize + 8) + L * (dtype.itemsize + 8)
                ok &= one("packed L=%d eos %s" % (L, str(dtype).rpartition(".")[2]), new,
                          lambda L=L, dtype=dtype: torch_collate_packed(ids, oo, n_ids, L, EOT, dtype), moved)
                packer.close()
        L = 256
        kept = int((oo[1:] - oo[:-1]).clamp_(max=L - 2).sum().item())
        moved = kept * 4 + (n_docs + 1) * 8 + n_docs * L * 5 + n_docs * 4
        ok &= one("padded L=256 right/right bos+eos int32",
                  lambda: H.collate_padded(ids, oo, L, bos_id=EOT, eos_id=EOT, pad_id=0, n_ids=n_ids),
                  lambda: torch_collate_padded(ids, oo, n_ids, L, EOT, EOT, 0, torch.int32), moved)
    p2048 = results["configs"][0]["new"]["median_ms"]
    results["loader_step_ms"] = {"encode": results["encode_step"]["median_ms"], "collate_packed_2048_int32": p2048,
                                 "sum": results["encode_step"]["median_ms"] + p2048}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        sys.exit("bench_collate: the HIP path is not faster than the torch composition in every configuration")


if __name__ == "__main__":
    main()
