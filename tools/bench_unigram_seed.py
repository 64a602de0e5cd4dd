#!/usr/bin/env python3
"""The seed of a Unigram training made on the GPU, device-resident, on the C3-shaped synthetic
corpus: ms a call and GB/s of UnigramSeeder.add beside the best-path pass with the golden vocabulary (the yardstick of a
pass bound by the same front half); the unique words and arena bytes of the corpus; the counting pass alone (ms, the
table's size and slots in use); the whole of pieces(); and train_unigram(texts, None, --vocab-size) wall time.  One JSON
line per figure in bench.py's style; a secondary measurement."""
import argparse, gzip, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import hutoken_amd
from hutoken_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--seed-size", type=int, default=30_000)
ap.add_argument("--vocab-size", type=int, default=3_000)
ap.add_argument("--no-fit", action="store_true")
ap.add_argument("--out")
args = ap.parse_args()
with gzip.open(os.path.join(ROOT, "tests", "golden", "unigram_vocab.json.gz"), "rt", encoding="utf-8") as f:
    g = json.load(f)
d, o = synth.corpus("C3", args.docs)
dev = torch.device("cuda", 0)
db, do = torch.from_numpy(np.ascontiguousarray(d)).to(dev), torch.from_numpy(np.ascontiguousarray(o)).to(dev)
workload = "C3 %d docs, %.1f MB of text, device-resident" % (args.docs, len(d) / 1e6)
results = []


def timed(what, fn, unit_bytes=None, **config):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.steps):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / args.steps
    res = {"metric": what, "ms_per_step": round(dt * 1e3, 3), "n_gpus": 1, "steps": args.steps, "config": dict(workload=workload, **config)}
    if unit_bytes:
        res.update(value=round(unit_bytes / dt / 1e9, 2), unit="GB/s")
    else:
        res.update(value=round(dt * 1e3, 3), unit="ms")
    results.append(res)
    print(json.dumps(res), flush=True)


ug = hutoken_amd.Unigram([(p, s) for p, s in g["vocab"]], g["unk_id"])
timed("Unigram.encode_packed_device, best path", lambda: ug.encode_packed_device(db, do), len(d))
seeder = hutoken_amd.UnigramSeeder()
seeder.add((db, do))  # (the first call claims every unique word; the timed ones find them all: the steady state of a stream)
info = seeder._h.info()
timed("UnigramSeeder.add, every word already in the table", lambda: seeder.add((db, do)), len(d), unique_words=info["n_words"],
      arena_bytes=info["arena_bytes"], word_slots=info["word_slots"], word_table_grows=info["word_table_grows"])
fresh = []


def first_add():
    if fresh:
        fresh.pop().close()
    fresh.append(hutoken_amd.UnigramSeeder().add((db, do)))


timed("UnigramSeeder.add, an empty table (create, grow, claim, settle)", first_add, len(d))
fresh.pop().close()
lines = seeder.pieces(args.seed_size)  # (finds the table size that holds the substrings)
slots = seeder._h.info()["substring_slots"]
out = torch.empty(2, dtype=torch.int64, device=dev)
stream = torch.cuda.current_stream(dev).cuda_stream or 0
timed("hutk_ugseed_count_device, substrings of 2 .. 16 characters", lambda: seeder._h.count_device(16, slots, out.data_ptr(), stream),
      substring_slots=slots, arena_bytes=info["arena_bytes"])
results[-1]["config"]["slots_in_use"] = int(out[1].item()) if out[0].item() == 0 else None  # (of the last pass)
timed("UnigramSeeder.pieces, seed_size=%d" % args.seed_size, lambda: seeder.pieces(args.seed_size), lines=len(lines))
seeder.close()
if not args.no_fit:
    raw = d.tobytes()
    texts = [raw[o[i]:o[i + 1]].decode("utf-8", "surrogateescape") for i in range(args.docs)]
    torch.cuda.synchronize()
    t = time.perf_counter()
    fitted = hutoken_amd.train_unigram(texts, None, args.vocab_size, seed_size=args.seed_size)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    res = {"metric": "train_unigram(texts, None, %d) wall time, packing and upload included" % args.vocab_size, "value": round(dt, 3), "unit": "s",
           "n_gpus": 1, "config": {"workload": workload, "seed_size": args.seed_size, "vocab_size": fitted.vocab_size}}
    results.append(res)
    print(json.dumps(res), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
