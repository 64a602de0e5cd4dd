#!/usr/bin/env python3
"""The byte-fallback encode (hutoken_amd.encode_fallback_packed_device, csrc/hutk_fallback.hip) against what a user of
encode_packed_device and token_spans_device composes today, on one GPU in one process.

C3 (1 M documents) under VL (characters, prefix, ids of -1), everything on device tensors, timed with device events,
warmed up, alternating, `--reps` times:

  (a) encode    the plain encode (encode_packed_device, check=False);
  (b) spans     (a), the one synchronising read of the number of ids, token_spans_device(unit="byte", check=False);
  (c) fallback  the fallback encode (check=False): plain encode, spans over the id CAPACITY (it never synchronises, so it
                never learns the number of ids), expansion;
  (d) torch     (b) and torch_expand below: counts, cumsum, repeat_interleave, gathers -- the same ids and offsets,
                asserted with torch.equal before anything is timed.

The expansion alone is (c) - (b) for the HIP path -- which charges it the spans of the unused capacity too -- and
(d) - (b) for torch.  Writes one JSON file (default profiles/fallback_bench.json); fails without a GPU.

  python tools/bench_fallback.py [--docs N] [--reps R] [--out FILE] [--head NAME]
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


def torch_expand(d_bytes, d_offs, ids, oo, spans, n_ids, table):
    """-> (expanded ids int32, out_offsets int64): every -1 becomes table[b] for the bytes b of its span."""
    import torch
    dev = ids.device
    n_docs = oo.numel() - 1
    idv = ids[:n_ids]
    unknown = idv < 0
    start = spans[:, 0].long()
    counts = torch.where(unknown, spans[:, 1].long() - start, torch.ones_like(start))
    pos = torch.cumsum(counts, 0)
    total = int(pos[-1].item()) if n_ids else 0
    src = torch.repeat_interleave(torch.arange(n_ids, device=dev), counts, output_size=total)
    within = torch.arange(total, device=dev) - (pos - counts)[src]
    doc = torch.repeat_interleave(torch.arange(n_docs, device=dev), oo[1:] - oo[:-1], output_size=n_ids)
    at = (d_offs[:-1][doc] + start)[src] + within
    fallback = table[d_bytes[at.clamp(max=d_bytes.numel() - 1)].long()]
    out = torch.where(unknown[src], fallback, idv[src])
    new_oo = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), pos])[oo]
    return out.to(torch.int32), new_oo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fallback_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fallback: no GPU; there is nothing to measure without one")
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
    d, o = synth.corpus("C3", args.docs)
    vp, sp, kw = data.vocab_files("VL")
    H.initialize(vp, sp, device=0, **kw)
    H.set_byte_fallback()
    table = torch.from_numpy(H.context().byte_fallback).to(dev)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_bytes, d_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)

        def encode():
            return H.encode_packed_device(d_bytes, d_offs, check=False)

        def spans():
            ids, oo = encode()
            n_ids = int(oo[-1].item())
            return ids, oo, n_ids, H.token_spans_device(d_bytes, d_offs, ids, oo, unit="byte", n_ids=n_ids, check=False)

        def fallback():
            return H.encode_fallback_packed_device(d_bytes, d_offs, check=False)

        def composed():
            ids, oo, n_ids, sp_ = spans()
            return torch_expand(d_bytes, d_offs, ids, oo, sp_, n_ids, table)

        ids, oo, n_ids, _sp = spans()
        unknown = int((ids[:n_ids] < 0).sum().item())
        got, goo = H.encode_fallback_packed_device(d_bytes, d_offs)
        want, woo = composed()
        torch.cuda.synchronize()
        n_out = int(woo[-1].item())
        assert torch.equal(goo, woo) and torch.equal(got[:n_out], want), "the HIP path and the torch composition differ"
        assert not bool((want < 0).any().item())
        del got, goo, want, woo, ids, oo, _sp
        torch.cuda.empty_cache()
        t = timed_alternating({"encode": encode, "spans": spans, "fallback": fallback, "torch": composed}, args.reps)
    r = {"git_head": head, "device": torch.cuda.get_device_name(0), "corpus": "C3", "vocab": "VL", "docs": args.docs,
         "bytes": int(o[-1]), "reps": args.reps, "ids": n_ids, "unknown_ids": unknown, "ids_out": n_out,
         "ids_capacity": int(H.context().ids_capacity(int(o[-1]), args.docs))}
    for k in t:
        r[k] = summary(t[k])
    r["expand_hip_ms"] = r["fallback"]["median_ms"] - r["spans"]["median_ms"]
    r["expand_torch_ms"] = r["torch"]["median_ms"] - r["spans"]["median_ms"]
    r["torch_spread_ms"] = r["torch"]["max_ms"] - r["torch"]["min_ms"]
    r["expand_hip_beats_torch_beyond_its_spread"] = r["expand_hip_ms"] < r["expand_torch_ms"] - r["torch_spread_ms"]
    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
