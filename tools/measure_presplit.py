#!/usr/bin/env python3
"""Cost of the split presets (pretokenize_packed_device and a context with a preset) on two
corpora of hutoken_amd.synth: C3 (Hungarian text) and cjk_paragraphs.

Per corpus: a device-to-device copy of the same bytes (torch.clone) as the yardstick -- the split reads the text once
and writes one bit per byte -- and, per preset, the split alone (the bitmap, enqueued), encode_packed_device with the
preset and without one on the same context, the tile-kernel time of both from hutk_last_timing, and the token counts
(they differ because the split differs).  HIP events, warm-up, the median of the timed iterations.

    python tools/measure_presplit.py --out profiles/presplit_throughput.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, warmup, iters):
    """median milliseconds of fn() by HIP events on the current stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000, help="documents of the C3 corpus")
    ap.add_argument("--cjk-docs", type=int, default=100000)
    ap.add_argument("--presets", default="gpt2,cl100k,qwen2")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default="profiles/presplit_throughput.json")
    args = ap.parse_args()
    import torch

    import hutoken_amd as hutoken
    from hutoken_amd import _capi, data, synth
    if not torch.cuda.is_available():
        raise SystemExit("measure_presplit: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    vp, sp, _kw = data.vocab_files("VG")
    hutoken.initialize(vp, sp, is_byte_encoder=True)
    ctx = hutoken.context()
    ctx.set_timing(True) if hasattr(ctx, "set_timing") else None
    res = {"device": torch.cuda.get_device_name(0), "vocabulary": "VG", "chunk_bytes": _capi.presplit_chunk_bytes(),
           "warmup": args.warmup, "iterations": args.iters, "statistic": "median, HIP events", "corpora": {}}
    corpora = [("c3", synth.corpus("C3", n_docs=args.docs)), ("cjk", synth.cjk_paragraphs(args.cjk_docs))]
    for name, (raw, offs) in corpora:
        db, do = torch.from_numpy(np.ascontiguousarray(raw)).to(dev), torch.from_numpy(np.ascontiguousarray(offs)).to(dev)
        n_bytes = int(offs[-1])
        entry = {"docs": len(offs) - 1, "bytes": n_bytes, "presets": {}}
        entry["copy_ms"] = timed(torch, lambda: db.clone(), args.warmup, args.iters)

        def encode():
            return hutoken.encode_packed_device(db, do, check=False)

        def tile_ms():
            try:
                return ctx.last_timing()[0]
            except Exception:  # (no timed call: the context was made without timing)
                return None

        hutoken.set_pretokenizer(None)
        entry["plain_encode_ms"] = timed(torch, encode, args.warmup, args.iters)
        entry["plain_tile_kernel_ms"] = tile_ms()
        entry["plain_tokens"] = int(encode()[1][-1])
        for preset in args.presets.split(","):
            p = {}
            p["split_ms"] = timed(torch, lambda: hutoken.pretokenize_packed_device(db, do, preset, return_bits=True), args.warmup, args.iters)
            p["split_gb_per_s"] = round(n_bytes / p["split_ms"] / 1e6, 1)
            p["split_over_copy"] = round(p["split_ms"] / entry["copy_ms"], 2)
            starts, _so = hutoken.pretokenize_packed_device(db, do, preset)
            p["words"] = int(starts.numel())
            hutoken.set_pretokenizer(preset)
            p["encode_ms"] = timed(torch, encode, args.warmup, args.iters)
            p["tile_kernel_ms"] = tile_ms()
            p["tokens"] = int(encode()[1][-1])
            p["encode_gb_per_s"] = round(n_bytes / p["encode_ms"] / 1e6, 1)
            hutoken.set_pretokenizer(None)
            entry["presets"][preset] = p
        entry["plain_encode_gb_per_s"] = round(n_bytes / entry["plain_encode_ms"] / 1e6, 1)
        res["corpora"][name] = entry
        del db, do
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
