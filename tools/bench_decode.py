#!/usr/bin/env python3
"""Decode direction, device-resident: ids + id_offsets in HBM -> text + out_offsets in HBM.
One JSON line in bench.py's style; a secondary measurement, not the BASELINE metric."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from hutoken_amd import _capi, data, synth

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--events", action="store_true", help="also time every step with device events: step_ms, step_ms_median")
args = ap.parse_args()
vp, sp, kw = data.vocab_files("VG")
ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"])
d, o = synth.corpus("C3", args.docs)
dev = torch.device("cuda", 0)
db, do = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
cap = ctx.ids_capacity(len(d), args.docs)
ids = torch.empty(cap, dtype=torch.int32, device=dev)
oo = torch.empty(args.docs + 1, dtype=torch.int64, device=dev)
err = torch.zeros(1, dtype=torch.int32, device=dev)
st = torch.cuda.current_stream().cuda_stream
ctx.encode_device(db.data_ptr(), do.data_ptr(), args.docs, len(d), ids.data_ptr(), cap, oo.data_ptr(), 0, err.data_ptr(), st)
torch.cuda.synchronize()
n_ids = int(oo[-1])
text = torch.empty(len(d) + 64, dtype=torch.uint8, device=dev)
boff = torch.empty(args.docs + 1, dtype=torch.int64, device=dev)


def step():
    ctx.decode_device(ids.data_ptr(), oo.data_ptr(), args.docs, n_ids, text.data_ptr(), len(d) + 64, boff.data_ptr(), 0,
                      err.data_ptr(), st)


for _ in range(args.warmup):
    step()
torch.cuda.synchronize()
assert int(err.item()) == 0
assert torch.equal(text[: len(d)], db) and torch.equal(boff, do), "decode(encode(text)) != text"
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps if args.events else 0)]
t = time.perf_counter()
for k in range(args.steps):
    if ev:
        ev[k][0].record()
    step()
    if ev:
        ev[k][1].record()
torch.cuda.synchronize()
dt = (time.perf_counter() - t) / args.steps
step_ms = sorted(round(a.elapsed_time(b), 4) for a, b in ev)
b_alg = 4 * n_ids + 8 * (args.docs + 1) + len(d) + 8 * (args.docs + 1)
print(json.dumps({"metric": "GB/s of text decoded (GPT-2-shaped vocab), bit-exact round trip", "value": round(len(d) / dt / 1e9, 2),
                  "unit": "GB/s", "ms_per_step": round(dt * 1e3, 4), "n_gpus": 1, "steps": args.steps,
                  **({"step_ms_median": step_ms[len(step_ms) // 2], "step_ms_min": step_ms[0], "step_ms_max": step_ms[-1]} if ev else {}),
                  "config": {"workload": f"C3 {args.docs} docs, {len(d)/1e6:.1f} MB of text, {n_ids} ids, device-resident"},
                  "roofline": {"bound": "hbm", "achieved": round(b_alg / dt / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                               "frac": round(b_alg / dt / 8e12, 4), "algorithmic_bytes": b_alg,
                               "note": "whole decode pipeline (memset, k_dec_pre, k_dec_tiles, k_dec_tail), dominated by k_dec_tiles"}}))
