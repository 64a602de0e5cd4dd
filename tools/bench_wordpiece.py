#!/usr/bin/env python3
"""WordPiece on the GPU, device-resident: GB/s of input text through
WordPiece.encode_packed_device on the C3-shaped synthetic corpus with the golden vocabulary, uncased and cased; and,
where `tokenizers` is importable, tokenizers.Tokenizer.encode_batch over texts of the same corpus on the same machine --
the host path a user has today.  One JSON line per setting in bench.py's style; a secondary measurement, not the
BASELINE metric.  --trace: five batches of one setting and nothing else (run under rocprofv3 --kernel-trace)."""
import argparse, gzip, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import hutoken_amd
from hutoken_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--host-docs", type=int, default=100_000, help="documents of the same corpus given to tokenizers (0: skip)")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--trace", choices=("uncased", "cased"))
ap.add_argument("--out", help="write the results as one JSON file as well")
args = ap.parse_args()
SETTINGS = {"uncased": dict(lowercase=True), "cased": dict(lowercase=False)}
with gzip.open(os.path.join(ROOT, "tests", "golden", "wordpiece_vocab.txt.gz"), "rt", encoding="utf-8", newline="\n") as f:
    lines = f.read().split("\n")[:-1]
d, o = synth.corpus("C3", args.docs)
dev = torch.device("cuda", 0)
db, do = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
results = {}
for name, opts in SETTINGS.items():
    if args.trace and name != args.trace:
        continue
    wp = hutoken_amd.WordPiece(lines, **opts)
    for _ in range(5 if args.trace else args.warmup):
        ids, oo = wp.encode_packed_device(db, do)
    torch.cuda.synchronize()
    if args.trace:
        print(len(d), "bytes", args.docs, "docs", ids.numel(), "ids")
        continue
    t = time.perf_counter()
    for _ in range(args.steps):
        ids, oo = wp.encode_packed_device(db, do)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / args.steps
    res = {"metric": "GB/s of text through WordPiece.encode_packed_device (%s, golden vocabulary)" % name,
           "value": round(len(d) / dt / 1e9, 2), "unit": "GB/s", "ms_per_step": round(dt * 1e3, 3), "n_gpus": 1, "steps": args.steps,
           "config": {"workload": "C3 %d docs, %.1f MB of text, %d ids, device-resident" % (args.docs, len(d) / 1e6, ids.numel())}}
    if args.host_docs:
        try:
            import tokenizers
        except ImportError:
            tokenizers = None
        if tokenizers is not None:
            n = min(args.host_docs, args.docs)
            raw = d[:o[n]].tobytes()
            texts = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(n)]
            vocab = {}
            for i, tkn in enumerate(lines):
                vocab[tkn] = i
            tok = tokenizers.Tokenizer(tokenizers.models.WordPiece(vocab, unk_token="[UNK]"))
            tok.normalizer = tokenizers.normalizers.BertNormalizer(**opts)
            tok.pre_tokenizer = tokenizers.pre_tokenizers.BertPreTokenizer()
            tok.encode_batch(texts[:1000], add_special_tokens=False)
            t = time.perf_counter()
            encs = tok.encode_batch(texts, add_special_tokens=False)
            ht = time.perf_counter() - t
            same = wp.batch_encode(texts[:2000]) == [e.ids for e in encs[:2000]]
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
