#!/usr/bin/env python3
"""GPU BPE training (hutoken_amd.Trainer) against tools/train_vocab.cpp on the same box, on the two configurations
that produced the committed vocabularies:

  VG  synth.corpus("C3", 125000, seed=0x564f4347), 50000 merges          (data/vg50257_*)
  VC  synth.cjk_text(8000, seed=0x56435452) split on "\\n", 12000 merges  (data/vc12257_vocab.txt.gz)

Phases timed separately: corpus generation, add (word count), run (merge loop; also its device time per merge), and the
CPU trainer's wall time (one process, single-threaded trainer; its VG run includes its own corpus generation).  The GPU
pairs are checked against the CPU trainer's.  Prints one JSON object.

  python tools/bench_train.py [--only VG|VC] [--no-cpu] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _cpu(exe, args, tmp):
    out, pf = os.path.join(tmp, "o.txt"), os.path.join(tmp, "p.txt")
    t0 = time.perf_counter()
    subprocess.run([exe, *args, out, "bytes", pf], check=False, capture_output=True)
    wall = time.perf_counter() - t0
    return wall, [tuple(bytes.fromhex(x) for x in ln.split()) for ln in open(pf)]


def _tokens(pairs):
    toks = [bytes([b]) for b in range(256)]
    for a, b in pairs:
        toks.append(toks[a] + toks[b])
    return [(toks[a], toks[b]) for a, b in pairs]


def run_config(name, cpu, exe, tmp):
    import numpy as np
    import hutoken_amd as H
    from hutoken_amd import synth
    t0 = time.perf_counter()
    if name == "VG":
        d, o = synth.corpus("C3", 125000, seed=0x564f4347)
        n_merges = 50000
    else:
        d0, o0 = synth.cjk_text(8000, seed=0x56435452)
        raw = d0.tobytes()
        pars = [p for i in range(len(o0) - 1) for p in raw[o0[i]:o0[i + 1]].split(b"\n")]
        d = np.frombuffer(b"".join(pars), dtype=np.uint8)
        o = np.zeros(len(pars) + 1, dtype=np.int64)
        o[1:] = np.cumsum([len(p) for p in pars])
        n_merges = 12000
    t_gen = time.perf_counter() - t0
    t = H.Trainer()
    t0 = time.perf_counter()
    t.add_packed(d, o)
    t_add = time.perf_counter() - t0
    t0 = time.perf_counter()
    pairs, counts = t.run(n_merges)
    t_run = time.perf_counter() - t0
    st = t.stats()
    t.close()
    res = {"config": name, "docs": int(len(o) - 1), "bytes": int(o[-1]), "merges": int(len(pairs)),
           "gen_s": round(t_gen, 3), "add_s": round(t_add, 4), "run_s": round(t_run, 4),
           "gpu_total_s": round(t_add + t_run, 4), "loop_us_per_merge": round(st["merge_loop_us"] / max(len(pairs), 1), 2),
           "stats": st}
    if cpu:
        if name == "VG":
            wall, cpp = _cpu(exe, ["3", "0x564f4347", "125000", str(n_merges)], tmp)
        else:
            path = os.path.join(tmp, "vc.txt")
            with open(path, "wb") as f:
                f.write(b"".join(bytes(d[o[i]:o[i + 1]]) + b"\n" for i in range(len(o) - 1)))
            wall, cpp = _cpu(exe, ["0", path, "0", str(n_merges)], tmp)
        res["cpu_trainer_s"] = round(wall, 3)
        res["pairs_equal_cpu"] = _tokens(pairs.tolist()) == cpp
        res["speedup_vs_cpu"] = round(wall / (t_add + t_run), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["VG", "VC"])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    exe = None
    if not a.no_cpu:
        import make_vocab
        exe = make_vocab.build_trainer(tmp)
    # warm up: library load, device init
    import hutoken_amd as H
    w = H.Trainer()
    w.add(["warm up warm up"])
    w.run(2)
    w.close()
    out = {"host_cpu": (open("/proc/cpuinfo").read().split("model name")[1].split("\n")[0].strip(": ")
                        if os.path.exists("/proc/cpuinfo") else ""),
           "results": [run_config(n, not a.no_cpu, exe, tmp) for n in (["VG", "VC"] if not a.only else [a.only])]}
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
