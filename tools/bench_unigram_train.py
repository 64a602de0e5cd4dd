#!/usr/bin/env python3
"""Unigram training on the GPU, device-resident, on the C3-shaped synthetic corpus: ms a call and
GB/s of the E-step with the golden vocabulary in both accumulation forms, beside the sampler's pass (alpha=0.1: the same
backward filter) and the best path; then UnigramTrainer.fit from a seed of about --seed-pieces lines (the golden
vocabulary's and the most frequent substrings of the corpus' words, counted on the host) down to --vocab-size, with its
wall time and corpus passes.  One JSON line per figure in bench.py's style; a secondary measurement."""
import argparse, collections, gzip, json, os, sys, time
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
ap.add_argument("--seed-pieces", type=int, default=30_000)
ap.add_argument("--vocab-size", type=int, default=3_000)
ap.add_argument("--count-docs", type=int, default=20_000, help="documents whose substrings are counted for the seed")
ap.add_argument("--no-fit", action="store_true")
ap.add_argument("--out")
args = ap.parse_args()
with gzip.open(os.path.join(ROOT, "tests", "golden", "unigram_vocab.json.gz"), "rt", encoding="utf-8") as f:
    g = json.load(f)
vocab, unk_id = [(p, s) for p, s in g["vocab"]], g["unk_id"]
d, o = synth.corpus("C3", args.docs)
dev = torch.device("cuda", 0)
db, do = torch.from_numpy(np.ascontiguousarray(d)).to(dev), torch.from_numpy(np.ascontiguousarray(o)).to(dev)
ug = hutoken_amd.Unigram(vocab, unk_id)
results = []


def timed(what, fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.steps):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / args.steps
    res = {"metric": what, "value": round(len(d) / dt / 1e9, 2), "unit": "GB/s", "ms_per_step": round(dt * 1e3, 3), "n_gpus": 1,
           "steps": args.steps, "config": {"workload": "C3 %d docs, %.1f MB of text, golden vocabulary, device-resident" % (args.docs, len(d) / 1e6)}}
    results.append(res)
    print(json.dumps(res), flush=True)


timed("Unigram.encode_packed_device, best path", lambda: ug.encode_packed_device(db, do))
timed("Unigram.encode_packed_device, alpha=0.1", lambda: ug.encode_packed_device(db, do, alpha=0.1, seed=1))
for acc in ("table", "atomics", "table"):
    timed("Unigram.expected_counts_device, accumulator=%s" % acc, lambda: ug.expected_counts_device(db, do, accumulator=acc))
if not args.no_fit:
    t = time.perf_counter()
    n = min(args.count_docs, args.docs)
    words = collections.Counter(("▁" + w) for w in d[:o[n]].tobytes().decode("utf-8", "replace").split())
    subs = collections.Counter()
    for w, c in words.items():
        for k in range(2, 9):
            for i in range(len(w) - k + 1):
                if "▁" not in w[i + 1:i + k]:
                    subs[w[i:i + k]] += c
    have = {p for p, _s in vocab}
    chars = sorted({c for w in words for c in w} - have)
    extra = [s for s, _c in subs.most_common() if s not in have][:max(args.seed_pieces - len(vocab) - len(chars), 0)]
    seed = [p for p, _s in vocab if "▁" not in p[1:] and " " not in p] + chars + extra
    seed = list(dict.fromkeys(seed))  # (the golden vocabulary holds one line twice)
    seed = [seed.pop(seed.index(vocab[unk_id][0]))] + seed
    host = time.perf_counter() - t
    trainer = hutoken_amd.UnigramTrainer(seed, 0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    fitted = trainer.fit((db, do), args.vocab_size)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    res = {"metric": "UnigramTrainer.fit wall time", "value": round(dt, 3), "unit": "s", "n_gpus": 1,
           "config": {"workload": "C3 %d docs, %.1f MB of text" % (args.docs, len(d) / 1e6), "seed_pieces": len(seed), "vocab_size": fitted.vocab_size,
                      "corpus_passes": trainer.passes, "seed_made_on_the_host_in_s": round(host, 2)}}
    results.append(res)
    print(json.dumps(res), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
