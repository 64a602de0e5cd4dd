#!/usr/bin/env python3
"""Span corruption on the GPU (hutoken_amd.corrupt_spans: k_rows_span_corrupt of csrc/hutk_collate.hip) against
torch.clone of its inputs plus its outputs: the floor for a pass that must read the rows and write these rectangles; the
method of tools/bench_targets.py.

C3 (1 M documents) is encoded once with VG and collated with an eos into int32 rows of 512: `padded`, a document a row,
and `dense`, all ids as ONE document in windows of 512 without stride, where every column but the eos is a token and
draws.  Timed with device events, 3 warm-up and `--reps` timed repetitions, the kernel and the clones alternating;
medians.  Bytes moved are computed from shapes.  Before anything is timed the outputs are checked against each other: the
round trip from the corrupted rows and the targets back to the rows, on the first 64 rows.

Every layout is a step of its own: a child process under its own time limit (`--limit` seconds), and nothing more is
started after a step that failed or ran out of time.  Writes one JSON file (default profiles/span_corrupt_bench.json); no
ratio is required.

  python tools/bench_span_corruption.py [--docs N] [--reps R] [--out FILE] [--head NAME] [--limit S]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

EOS, FIRST, L = 50256, 50356, 512
DENSITY, MEAN, MAX_SPAN = 0.15, 3.0, 10
LAYOUTS = ("padded", "dense")


def round_trip(rows, mask, out, in_len, labels, tgt_len, n=64):
    """the first n rows rebuilt from the outputs alone"""
    rows, mask, out, in_len, labels, tgt_len = (x[:n].cpu().numpy() for x in (rows, mask, out, in_len, labels, tgt_len))
    for r in range(len(rows)):
        spans, key = {}, None
        assert tgt_len[r] <= labels.shape[1] and labels[r, tgt_len[r] - 1] == EOS
        for x in labels[r, :tgt_len[r] - 1].tolist():  # (the eos closes the target)
            if x > FIRST - 100:
                key = x
                spans[key] = []
            else:
                spans[key].append(x)
        got = []
        for x in out[r, :in_len[r]].tolist():
            got += spans.pop(x) if x > FIRST - 100 else [x]
        assert not spans and got == rows[r][mask[r] != 0].tolist(), r


def step(layout, docs, reps, part):
    """one layout, in this process -> its record, written to `part`"""
    import torch
    from bench_collate import summary, timed_alternating
    import hutoken_amd as H
    from hutoken_amd import data, synth
    dev = torch.device("cuda", 0)
    vp, sp, _kw = data.vocab_files("VG")
    H.initialize(vp, sp, is_byte_encoder=True)
    d, o = synth.corpus("C3", docs)
    st = torch.cuda.Stream(dev)  # a stream of torch's own: every call here is then ordered with the others
    with torch.cuda.stream(st):
        ids, oo = H.encode_packed_device(torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev))
        n_ids = int(oo[-1].item())
        if layout == "padded":
            rows, mask, lengths, plan = H.collate_padded(ids, oo, L, eos_id=EOS, n_ids=n_ids, return_plan=True, check=True)
        else:
            one = torch.tensor([0, n_ids], dtype=torch.int64, device=dev)
            rows, mask, lengths, _row_map, plan = H.collate_windows(ids, one, L, 0, eos_id=EOS, n_ids=n_ids, return_plan=True, check=True)
        del ids, oo
        n_rows = rows.shape[0]
        eligible = int(lengths.sum().item()) - n_rows  # every row has its eos
        kw = dict(sentinel_first=FIRST, noise_density=DENSITY, mean_span_length=MEAN, max_span_length=MAX_SPAN, target_eos_id=EOS)
        got = H.corrupt_spans(rows, mask, plan, seed=1, check=True, **kw)
        round_trip(rows, mask, got[0], got[3], got[2], got[4])
        # noise columns = real columns - kept columns + runs; target elements = noise columns + runs + 1 (eos)
        real, kept, targets = int(lengths.sum().item()), int(got[3].sum().item()), int(got[4].sum().item()) - n_rows
        runs = (targets - (real - kept)) // 2
        noise = real - kept + runs
        seeds = iter(range(2, 10**6))
        rect = n_rows * L * 4
        moved = (rect + n_rows * L + n_rows * 64) + (rect + n_rows * L + rect + n_rows * 8)  # read: ids, mask, plan; written: ids, mask, labels, lengths
        fns = {"new": lambda: H.corrupt_spans(rows, mask, plan, seed=next(seeds), **kw),
               "clone": lambda: (rows.clone(), mask.clone(), got[0].clone(), got[1].clone(), got[2].clone())}
        t = timed_alternating(fns, reps)
    rec = {"layout": layout, "rows": n_rows, "ids": n_ids, "eligible_columns": eligible, "fill": eligible / (n_rows * L),
           "noise_fraction_of_eligible": noise / eligible, "runs_per_row": runs / n_rows, "bytes_moved": moved,
           "clone_bytes_moved": 2 * (3 * rect + 2 * n_rows * L), "device": torch.cuda.get_device_name(0)}
    for k, ms in t.items():
        rec[k] = summary(ms)
    rec["new_GBps"] = moved / rec["new"]["median_ms"] / 1e6
    rec["clone_GBps"] = rec["clone_bytes_moved"] / rec["clone"]["median_ms"] / 1e6
    rec["ratio_new_over_clone"] = rec["new"]["median_ms"] / rec["clone"]["median_ms"]
    with open(part, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "span_corrupt_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    ap.add_argument("--limit", type=int, default=240, help="seconds a layout's step may take")
    ap.add_argument("--layout", choices=LAYOUTS, default=None, help="(a step: this layout alone, in this process)")
    ap.add_argument("--part", default=None, help="(a step: where its record goes)")
    args = ap.parse_args()
    if args.layout:
        return step(args.layout, args.docs, args.reps, args.part)
    head = args.head
    if head is None:
        try:
            head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            head = "unknown"
    results = {"git_head": head, "corpus": "C3", "vocab": "VG", "docs": args.docs, "max_length": L, "dtype": "int32", "reps": args.reps,
               "warmup": 3, "noise_density": DENSITY, "mean_span_length": MEAN, "max_span_length": MAX_SPAN, "layouts": []}
    with tempfile.TemporaryDirectory() as tmp:
        for layout in LAYOUTS:
            part = os.path.join(tmp, layout + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--layout", layout, "--part", part, "--docs", str(args.docs), "--reps", str(args.reps)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                sys.exit("bench_span_corruption: the step %r ran out of its %d s; nothing more is started" % (layout, args.limit))
            if rc:
                sys.exit("bench_span_corruption: the step %r ended with status %d; nothing more is started" % (layout, rc))
            with open(part) as f:
                results["layouts"].append(json.load(f))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
