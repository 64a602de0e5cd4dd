#!/usr/bin/env python3
"""BPE-dropout against the plain encoder on one GPU -> profiles/dropout_bench.json.

  python tools/bench_dropout.py [--docs N] [--steps 10] [--warmup 3] [--p 0.1] [--parent-lib OTHER.so --pairs 5] [--out FILE]

Throughput: C3 x VG, device-resident; encode_packed_device plain and with dropout=p alternate in ONE process, `warmup`
untimed steps of each first, every step between two device events.  Then the long form's worst case: one word of 262144
bytes that merges at every step.  With --parent-lib: bench.py --gpus 1 on that library
and on this tree's, alternating, the other library first, `pairs` pairs -- the plain path's figures side by side."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def throughput(docs, steps, warmup, p):
    import torch

    import hutoken_amd
    from hutoken_amd import data, synth
    vp, sp, kw = data.vocab_files("VG")
    hutoken_amd.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", docs)
    db, do = torch.from_numpy(d[:int(o[-1])].copy()).to("cuda:0"), torch.from_numpy(o).to("cuda:0")
    forms = {"plain": {}, "dropout": dict(dropout=p, seed=1)}
    ms, n_ids = {k: [] for k in forms}, {}
    with torch.cuda.stream(torch.cuda.Stream("cuda:0")):
        for step in range(warmup + steps):
            for name, kw in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _ids, oo = hutoken_amd.encode_packed_device(db, do, check=step == 0, **kw)  # (a refusal shows in the first, untimed step)
                b.record()
                b.synchronize()
                n_ids[name] = int(oo[-1].item())
                if step >= warmup:
                    ms[name].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"workload": "C3 x VG, device-resident", "docs": docs, "bytes": int(o[-1]), "p": p, "steps": steps, "warmup": warmup,
            "ms": ms, "median_ms": med, "GB_per_s": {k: int(o[-1]) / v / 1e6 for k, v in med.items()},
            "ratio_dropout_over_plain": med["dropout"] / med["plain"], "ids": n_ids, "ids_added": n_ids["dropout"] - n_ids["plain"]}


def long_word(n=262144, ps=(0.0, 0.5, 0.9)):
    """The long form's worst case: ONE word of n bytes that merges at every step ("a" repeated, under VG), second of two calls."""
    import numpy as np
    import torch

    import hutoken_amd
    db = torch.from_numpy(np.frombuffer(b"a" * n, dtype=np.uint8).copy()).to("cuda:0")
    do = torch.tensor([0, n], dtype=torch.int64, device="cuda:0")
    rows = []
    with torch.cuda.stream(torch.cuda.Stream("cuda:0")):
        for p in ps:
            for _rep in range(2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ids, oo = hutoken_amd.encode_packed_device(db, do, dropout=p, seed=1)
                b.record()
                b.synchronize()
            rows.append({"p": p, "bytes": n, "ms": a.elapsed_time(b), "ids": int(oo[-1].item())})
            if p == 0:
                pi, po = hutoken_amd.encode_packed_device(db, do)
                rows[-1]["equals_plain"] = bool(torch.equal(pi[:int(po[-1])], ids[:int(oo[-1])]))
    return rows


def plain_path(parent_lib, pairs, steps, warmup):
    """bench.py on the other library and on this tree's, the other first -> both series of `value` (GB/s)"""
    from hutoken_amd import _capi
    libs, series = {"parent": os.path.abspath(parent_lib), "tree": _capi.library_path()}, {"parent": [], "tree": []}
    for _pair in range(pairs):
        for name, lib in libs.items():
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                                 env=dict(os.environ, HUTOKEN_AMD_LIB=lib), capture_output=True, text=True, check=True).stdout
            series[name].append(json.loads(out.strip().splitlines()[-1])["value"])
    return {"cmd": "bench.py --gpus 1 --steps %d --warmup %d" % (steps, warmup), "unit": "GB/s", **series}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_bench.json"))
    args = ap.parse_args()
    res = {}
    if args.parent_lib:  # first: this process has not opened the GPU yet
        res["plain_path"] = plain_path(args.parent_lib, args.pairs, args.steps, args.warmup)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    res["throughput"] = throughput(args.docs, args.steps, args.warmup, args.p)
    res["long_word"] = long_word()  # (the context throughput() made)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res["throughput"].items() if k != "ms"}))


if __name__ == "__main__":
    main()
