#!/usr/bin/env python3
"""Packed rows for training (SequencePacker channels, packed_cu_seqlens, packed_lm_labels) against
what a user writes without them, on one GPU in one process, in the manner of tools/bench_collate.py: the same batch (C3,
1 M documents, encoded once with VG through encode_packed_device), device events, 3 warm-up and `--reps` timed
repetitions, the compared forms alternating, torch.equal asserted on every compared output before anything is timed.

  channel    one add() that carries an int32 channel, against two plain packers of equal geometry, one fed the ids and one
             fed the values (the recipe the README gave before channels existed); seq_len 2048 and 8192, no bos/eos
  cu         packed_cu_seqlens with a given cap, against the torch composition: compare with the shifted neighbour,
             nonzero, cat -- which synchronises (nonzero's output size is data)
  labels     packed_lm_labels(shift=True), against its torch composition and against one Tensor.copy_ of the bytes it moves

Writes one JSON file (default profiles/packed_bench.json).

  python tools/bench_packed.py [--docs N] [--reps R] [--out FILE] [--head NAME]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_collate import summary, timed_alternating  # noqa: E402

IGN = -100


def torch_cu_seqlens(seg):
    import torch
    start = torch.ones_like(seg, dtype=torch.bool)
    start[:, 1:] = seg[:, 1:] != seg[:, :-1]
    starts = start.view(-1).nonzero().view(-1).to(torch.int32)  # (synchronises: the size of the result is data)
    return torch.cat([starts, torch.tensor([seg.numel()], dtype=torch.int32, device=seg.device)])


def torch_labels_shift(values, seg, ignore):
    import torch
    out = torch.full_like(values, ignore)
    keep = (seg[:, 1:] == seg[:, :-1]) & (seg[:, :-1] != 0)
    out[:, :-1] = torch.where(keep, values[:, 1:], out[:, :-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_packed: no GPU; there is nothing to measure without one")
    import hutoken_amd as H
    from hutoken_amd import data, synth
    head = args.head
    if head is None:
        try:
            head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                           stderr=subprocess.DEVNULL).strip()
        except Exception:
            head = "unknown"
    dev = torch.device("cuda", 0)
    vp, sp, kw = data.vocab_files("VG")
    H.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", args.docs)
    st = torch.cuda.Stream(dev)
    results = {"git_head": head, "device": torch.cuda.get_device_name(0), "corpus": "C3", "vocab": "VG", "docs": args.docs,
               "bytes": int(o[-1]), "reps": args.reps, "configs": []}

    def record(label, fns, moved=None, **extra):
        t = timed_alternating(fns, args.reps)
        r = {"config": label, **{k: summary(v) for k, v in t.items()}, **extra}
        names = list(fns)
        for other in names[1:]:
            r["ratio_%s_over_%s" % (names[0], other)] = r[names[0]]["median_ms"] / r[other]["median_ms"]
        r["below_1_outside_the_baselines_spread"] = r["ratio_%s_over_%s" % (names[0], names[1])] < 1 - r[names[1]]["spread"]
        if moved is not None:
            r["bytes_moved"] = moved
            r["%s_GBps" % names[0]] = moved / r[names[0]]["median_ms"] / 1e6
        results["configs"].append(r)
        print(json.dumps(r), flush=True)

    with torch.cuda.stream(st):
        d_bytes, d_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
        ids, oo = H.encode_packed_device(d_bytes, d_offs)
        n_ids = int(oo[-1].item())
        results["ids"] = n_ids
        values = ids * 3 + 1  # an int32 channel along the ids
        rows_2048 = None
        for L in (2048, 8192):
            one = H.SequencePacker(L, pad_id=0, channels={"v": ("int32", IGN)})
            p_ids, p_val = H.SequencePacker(L, pad_id=0), H.SequencePacker(L, pad_id=IGN)

            def channel(one=one):
                rows = one.add(ids, oo, n_ids=n_ids, channels={"v": values})
                one.flush()  # every repetition packs the same stream from its start
                return rows["input_ids"], rows["position_ids"], rows["segment_ids"], rows["v"]

            def two(p_ids=p_ids, p_val=p_val):
                a, b = p_ids.add(ids, oo, n_ids=n_ids), p_val.add(values, oo, n_ids=n_ids)
                p_ids.flush()
                p_val.flush()
                return a["input_ids"], a["position_ids"], a["segment_ids"], b["input_ids"]

            got, want = channel(), two()
            torch.cuda.synchronize()
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), L
            if L == 2048:
                rows_2048 = {"input_ids": got[0].clone(), "segment_ids": got[2].clone()}
            del got, want
            record("one add with an int32 channel against two plain packers, L=%d" % L, {"channel": channel, "two_packers": two})
            for p in (one, p_ids, p_val):
                p.close()

        seg, row_ids = rows_2048["segment_ids"], rows_2048["input_ids"]
        n = seg.numel()
        want = torch_cu_seqlens(seg)
        n_seq = want.numel() - 1
        cap = n_seq + 1024
        cu, info = H.packed_cu_seqlens(seg, cap=cap)
        torch.cuda.synchronize()
        assert torch.equal(cu[:n_seq + 1], want) and bool((cu[n_seq:] == n).all()) and int(info[0]) == n_seq
        assert int(info[1]) == int((want[1:] - want[:-1]).max())
        record("packed_cu_seqlens with a given cap against compare, nonzero, cat; rows of L=2048",
               {"new": lambda: H.packed_cu_seqlens(seg, cap=cap), "torch": lambda: torch_cu_seqlens(seg)},
               moved=n * 4 + (cap + 1) * 4, n_seq=n_seq, torch_form_synchronises=True)

        got, want = H.packed_lm_labels(row_ids, seg, shift=True), torch_labels_shift(row_ids, seg, IGN)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        del got, want
        moved = n * 12  # values and segments read, labels written
        half = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        other = torch.empty_like(half)
        record("packed_lm_labels(shift=True) against its torch composition and one copy_ of its bytes; rows of L=2048",
               {"new": lambda: H.packed_lm_labels(row_ids, seg, shift=True), "torch": lambda: torch_labels_shift(row_ids, seg, IGN),
                "copy": lambda: other.copy_(half)}, moved=moved)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
