#!/usr/bin/env python3
"""Unigram on the GPU, device-resident: GB/s of input text through Unigram.encode_packed_device on
the C3-shaped synthetic corpus with the golden vocabulary, in metaspace and whitespace_split shape; the same corpus with
its spaces removed (every document one word: the long-word regime, reported separately); and, where `tokenizers` is
importable, tokenizers.Tokenizer.encode_batch over texts of the same corpus on the same machine -- the host path a user
has today.  One JSON line per case in bench.py's style; a secondary measurement, not the BASELINE metric.
--trace: five batches of one case and nothing else (run under rocprofv3 --kernel-trace)."""
import argparse, gzip, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import hutoken_amd
from hutoken_amd import synth

CASES = {"metaspace": dict(), "whitespace_split": dict(whitespace_split=True), "no_spaces": dict()}
ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--host-docs", type=int, default=100_000, help="documents of the same corpus given to tokenizers (0: skip)")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--trace", choices=sorted(CASES))
ap.add_argument("--out", help="write the results as one JSON file as well")
args = ap.parse_args()
with gzip.open(os.path.join(ROOT, "tests", "golden", "unigram_vocab.json.gz"), "rt", encoding="utf-8") as f:
    g = json.load(f)
vocab, unk_id = [(p, s) for p, s in g["vocab"]], g["unk_id"]
d, o = synth.corpus("C3", args.docs)
dev = torch.device("cuda", 0)
results = {}
for name, opts in CASES.items():
    if args.trace and name != args.trace:
        continue
    data, offs = d, o
    if name == "no_spaces":  # every document becomes one word
        keep = d != 0x20
        before = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
        data, offs = d[keep], before[o]
    db, do = torch.from_numpy(np.ascontiguousarray(data)).to(dev), torch.from_numpy(np.ascontiguousarray(offs)).to(dev)
    ug = hutoken_amd.Unigram(vocab, unk_id, **opts)
    for _ in range(5 if args.trace else args.warmup):
        ids, oo = ug.encode_packed_device(db, do)
    torch.cuda.synchronize()
    if args.trace:
        print(len(data), "bytes", args.docs, "docs", ids.numel(), "ids")
        continue
    t = time.perf_counter()
    for _ in range(args.steps):
        ids, oo = ug.encode_packed_device(db, do)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / args.steps
    res = {"metric": "GB/s of text through Unigram.encode_packed_device (%s, golden vocabulary)" % name,
           "value": round(len(data) / dt / 1e9, 2), "unit": "GB/s", "ms_per_step": round(dt * 1e3, 3), "n_gpus": 1, "steps": args.steps,
           "config": {"workload": "C3 %d docs, %.1f MB of text, %d ids, device-resident" % (args.docs, len(data) / 1e6, ids.numel())}}
    if args.host_docs and name != "no_spaces":
        try:
            import tokenizers
        except ImportError:
            tokenizers = None
        if tokenizers is not None:
            from tokenizers import models, pre_tokenizers
            n = min(args.host_docs, args.docs)
            raw = d[:o[n]].tobytes()
            texts = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(n)]
            tok = tokenizers.Tokenizer(models.Unigram(vocab, unk_id, False))
            ms = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always", split=True)
            tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.WhitespaceSplit(), ms]) if opts else ms
            tok.encode_batch(texts[:1000], add_special_tokens=False)
            t = time.perf_counter()
            encs = tok.encode_batch(texts, add_special_tokens=False)
            ht = time.perf_counter() - t
            same = ug.batch_encode(texts[:2000]) == [e.ids for e in encs[:2000]]
            res["host"] = {"what": "tokenizers %s Tokenizer.encode_batch, %d docs of the same corpus, %s" %
                           (tokenizers.__version__, n, "RAYON_NUM_THREADS=%s" % os.environ["RAYON_NUM_THREADS"]
                            if os.environ.get("RAYON_NUM_THREADS") else "its default thread pool"),
                           "value": round(int(o[n]) / ht / 1e9, 4), "unit": "GB/s", "seconds": round(ht, 3), "same_ids_on_2000_docs": same}
    results[name] = res
    print(json.dumps(res))
if args.out and results:
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
