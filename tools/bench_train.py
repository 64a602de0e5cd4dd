#!/usr/bin/env python3
"""GPU BPE training (hutoken_amd.Trainer) against tools/train_vocab.cpp on the same box, on the configurations that
produced the committed vocabularies:

  VG   bytes mode: synth.corpus("C3", 125000, seed=0x564f4347), 50000 merges          (data/vg50257_*)
  VC   bytes mode: synth.cjk_text(8000, seed=0x56435452) split on "\\n", 12000 merges  (data/vc12257_vocab.txt.gz)
  VL   chars mode: synth.corpus("C5", 60000, seed=0x564f434c), 31684 merges           (data/vl32000_vocab.txt.gz)
  CJK  chars mode: VC's corpus, 12000 merges

Phases timed separately: corpus generation, add (word count), alphabet (chars mode only: the symbolisation; in bytes
mode it stays inside run, as it always was), run (merge loop; also its device time per merge), and the CPU trainer's
wall time (one process, single-threaded trainer; its VG and VL runs include its own corpus generation).  The GPU pairs
(and in chars mode the alphabet) are checked against the CPU trainer's.  Prints one JSON object.

  python tools/bench_train.py [--only VG|VC|VL|CJK] [--no-cpu] [--out FILE]
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

CONFIGS = {"VG": "bytes", "VC": "bytes", "VL": "chars", "CJK": "chars"}


def _cpu(exe, args, tmp, mode):
    """-> (wall s, alphabet [bytes] (chars mode) or None, merges [(left bytes, right bytes)])."""
    out, pf = os.path.join(tmp, "o.txt"), os.path.join(tmp, "p.txt")
    t0 = time.perf_counter()
    subprocess.run([exe, *args, out, mode, pf], check=False, capture_output=True)
    wall = time.perf_counter() - t0
    base = [bytes.fromhex(x) for x in open(out).read().split("--\n")[0].split()] if mode == "chars" else None
    return wall, base, [tuple(bytes.fromhex(x) for x in ln.split()) for ln in open(pf)]


def _tokens(pairs, alphabet):
    toks = list(alphabet)
    for a, b in pairs:
        toks.append(toks[a] + toks[b])
    return [(toks[a], toks[b]) for a, b in pairs]


def run_config(name, cpu, exe, tmp):
    import numpy as np
    import hutoken_amd as H
    from hutoken_amd import synth
    mode = CONFIGS[name]
    t0 = time.perf_counter()
    if name == "VG":
        d, o = synth.corpus("C3", 125000, seed=0x564f4347)
        n_merges = 50000
    elif name == "VL":
        d, o = synth.corpus("C5", 60000, seed=0x564f434c)
        n_merges = 31684
    else:
        d0, o0 = synth.cjk_text(8000, seed=0x56435452)
        raw = d0.tobytes()
        pars = [p for i in range(len(o0) - 1) for p in raw[o0[i]:o0[i + 1]].split(b"\n")]
        d = np.frombuffer(b"".join(pars), dtype=np.uint8)
        o = np.zeros(len(pars) + 1, dtype=np.int64)
        o[1:] = np.cumsum([len(p) for p in pars])
        n_merges = 12000
    t_gen = time.perf_counter() - t0
    t = H.Trainer(mode=mode)
    t0 = time.perf_counter()
    t.add_packed(d, o)
    t_add = time.perf_counter() - t0
    t_alpha = 0.0
    if mode == "chars":
        t0 = time.perf_counter()
        alphabet = t.alphabet()
        t_alpha = time.perf_counter() - t0
    else:
        alphabet = [bytes([b]) for b in range(256)]
    t0 = time.perf_counter()
    pairs, counts = t.run(n_merges)
    t_run = time.perf_counter() - t0
    st = t.stats()
    t.close()
    total = t_add + t_alpha + t_run
    res = {"config": name, "mode": mode, "docs": int(len(o) - 1), "bytes": int(o[-1]), "merges": int(len(pairs)),
           "alphabet_size": len(alphabet), "gen_s": round(t_gen, 3), "add_s": round(t_add, 4),
           "alphabet_s": round(t_alpha, 4), "run_s": round(t_run, 4), "gpu_total_s": round(total, 4),
           "loop_us_per_merge": round(st["merge_loop_us"] / max(len(pairs), 1), 2), "stats": st}
    if cpu:
        if name == "VG":
            wall, base, cpp = _cpu(exe, ["3", "0x564f4347", "125000", str(n_merges)], tmp, mode)
        elif name == "VL":
            wall, base, cpp = _cpu(exe, ["5", "0x564f434c", "60000", str(n_merges)], tmp, mode)
        else:
            path = os.path.join(tmp, "vc.txt")
            with open(path, "wb") as f:
                f.write(b"".join(bytes(d[o[i]:o[i + 1]]) + b"\n" for i in range(len(o) - 1)))
            wall, base, cpp = _cpu(exe, ["0", path, "0", str(n_merges)], tmp, mode)
        res["cpu_trainer_s"] = round(wall, 3)
        res["pairs_equal_cpu"] = (base is None or base == alphabet) and _tokens(pairs.tolist(), alphabet) == cpp
        res["speedup_vs_cpu"] = round(wall / total, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=list(CONFIGS))
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
           "results": [run_config(n, not a.no_cpu, exe, tmp) for n in ([a.only] if a.only else list(CONFIGS))]}
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
