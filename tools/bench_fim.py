#!/usr/bin/env python3
"""Fill-in-the-middle on the GPU (hutoken_amd.fim_device / fim_cut_text_device, csrc/hutk_collate.hip) next to what a
user of encode_packed_device composes today, on one GPU in one process.

The batch of tools/bench_collate.py -- C3 (1 M documents) encoded once with VG -- is rendered at token level with
fim_rate = spm_rate = 0.5 and an end sentinel; then six things are timed with device events, warmed up (3), alternating,
`--reps` (20) times each:

  (a) fim      fim_device: the plan (count, scan, write, plan rows, kinds) plus the fill, ids + labels;
  (b) fim all  the same with all four outputs (ids, labels, parts, source);
  (c) torch    torch_fim below: the same four outputs composed from torch ops (cumsum, repeat_interleave, where, index
               reads), asserted equal to (b) on every output before anything is timed.  It is GIVEN the kinds and the
               cuts that (b) drew -- a composition of its own would draw them with randint and could not be compared --
               so it is timed without any draw;
  (d) packed   SequencePacker.add + flush over the same ids and offsets (seq_len 2048, int32): the yardstick of the chat
               section, with its own bytes moved;
  (e) cut      fim_cut_text_device over the batch's text alone;
  (f) plan     the plan call of (a) and (b) alone (count, scan, write, plan rows and kinds: four launches), which says
               how much of (a) and (b) is the fill.

Bytes moved follow the traffic model of DESIGN.md section 8k: 4 n_ids in, 4 n_out per int32 output and 8 n_out for the
source out, 8 bytes of offsets in and 8 + 32 + 4 bytes of out_offsets, plan and kinds out and in again per document.
Writes one JSON file (default profiles/fim_bench.json) and fails when (b) is not faster than (c) by more than (c)'s
spread.

  python tools/bench_fim.py [--docs N] [--reps R] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

IGNORE = -100
PRE, SUF, MID, END = 50257, 50258, 50259, 50260
SEED = 1234


def torch_fim(ids, offsets, kinds, lo, hi, n_ids, loss_parts):
    """(out_ids, out_offsets, labels, parts, source) of the rule in include/hutoken_amd.h, with an end sentinel"""
    import torch
    dev = ids.device
    n_docs = offsets.numel() - 1
    n = offsets[1:] - offsets[:-1]
    lens = torch.where(kinds == 0, n, n + 4)
    oo = torch.zeros(n_docs + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=oo[1:])
    n_out = int(oo[-1].item())
    p = torch.arange(n_out, device=dev)
    d = torch.repeat_interleave(torch.arange(n_docs, device=dev), lens, output_size=n_out)
    q = p - oo[d]
    k, nd, P, H = kinds[d], n[d], lo[d], hi[d]
    S = nd - H
    spm = k == 2
    # where the suffix begins and where mid stands: PSM  pre P suf S mid M end; SPM  pre suf S mid P M end
    suf_at = torch.where(spm, torch.ones_like(P), P + 1)
    mid_at = suf_at + S + 1
    is_sent = (k != 0) & ((q == 0) | (q == suf_at) | (q == mid_at) | (q == nd + 3))
    in_suffix = (q > suf_at) & (q < mid_at)
    behind_mid = q - mid_at - 1                                     # PSM: into the middle; SPM: into prefix + middle
    idx = torch.where(k == 0, q,
                      torch.where(in_suffix, H + q - suf_at - 1,
                                  torch.where(q > mid_at, torch.where(spm, behind_mid, P + behind_mid), q - 1)))
    part = torch.where(k == 0, torch.zeros_like(k),
                       torch.where(is_sent, torch.full_like(k, 4),
                                   torch.where(in_suffix, torch.full_like(k, 3),
                                               torch.where(idx < P, torch.ones_like(k), torch.full_like(k, 2)))))
    sent = torch.where(q == 0, PRE, torch.where(q == suf_at, SUF, torch.where(q == mid_at, MID, END))).to(torch.int32)
    src = offsets[d] + idx
    out = torch.where(is_sent, sent, ids[src.clamp(0, max(n_ids - 1, 0))])
    source = torch.where(is_sent, torch.tensor(-1, dtype=torch.int64, device=dev), src)
    bits = torch.tensor(loss_parts, dtype=torch.int64, device=dev)
    carries = ((bits >> part) & 1).bool() | (is_sent & (q == nd + 3) & ((bits >> 5) & 1).bool())
    labels = torch.where(carries, out, torch.tensor(IGNORE, dtype=torch.int32, device=dev))
    return out, oo, labels, part, source


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fim_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fim: no GPU; there is nothing to measure without one")
    import hutoken_amd as H
    from hutoken_amd import _capi, data, synth
    from bench_collate import summary, timed_alternating
    dev = torch.device("cuda", 0)
    vp, sp, kw = data.vocab_files("VG")
    H.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", args.docs)
    sent = dict(prefix_id=PRE, suffix_id=SUF, middle_id=MID, end_id=END)
    results = {"device": torch.cuda.get_device_name(0), "corpus": "C3", "vocab": "VG", "docs": args.docs, "bytes": int(o[-1]),
               "reps": args.reps, "fim_rate": 0.5, "spm_rate": 0.5, "seed": SEED, "span": _capi.fim_span()}
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_bytes, d_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
        ids, oo = H.encode_packed_device(d_bytes, d_offs)
        n_docs, n_ids = oo.numel() - 1, int(oo[-1].item())

        def fim(everything):
            return H.fim_device(ids, oo, seed=SEED, n_ids=n_ids, loss_on="middle", return_labels=True, return_parts=everything,
                                return_source=everything, **sent)

        # the kinds and the cuts of the batch, for the torch composition: the plan call on buffers of this tool's
        plan = torch.empty((n_docs, 4), dtype=torch.int64, device=dev)
        kinds = torch.empty(n_docs, dtype=torch.int32, device=dev)
        scratch = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        _capi.fim_plan_tokens_device(oo.data_ptr(), n_docs, n_ids, SEED, 0, 2**31, 2**31, True, scratch.data_ptr(), plan.data_ptr(),
                                     kinds.data_ptr(), 0, st.cuda_stream)
        k64, lo, hi = kinds.long(), plan[:, 2].contiguous(), plan[:, 3].contiguous()
        loss_bits = (1 << 0) | (1 << 2) | 32  # "middle": the middle, the end sentinel, plain documents
        want = torch_fim(ids, oo, k64, lo, hi, n_ids, loss_bits)
        got = fim(True)
        n_out = int(got[1][-1].item())
        assert torch.equal(got[1], want[1]) and torch.equal(got[1], scratch)
        for name, g, w in zip(("ids", "labels", "parts", "source"), (got[0], got[2], got[3], got[4]), (want[0], want[2], want[3].to(torch.int32), want[4])):
            assert g.dtype == w.dtype and torch.equal(g[:n_out], w), "the torch composition and the render differ in the %s" % name
        del got, want
        results.update(ids=n_ids, rendered_ids=n_out, transformed=int((kinds != 0).sum().item()), spm=int((kinds == 2).sum().item()))
        L = 2048
        packer = H.SequencePacker(L)

        def packed():
            rows = packer.add(ids, oo, n_ids=n_ids)
            packer.flush()  # every repetition packs the same stream from its start
            return rows

        fns = {"fim": lambda: fim(False), "fim_all": lambda: fim(True),
               "torch": lambda: torch_fim(ids, oo, k64, lo, hi, n_ids, loss_bits), "packed": packed,
               "cut": lambda: H.fim_cut_text_device(d_bytes, d_offs, seed=SEED),
               "plan": lambda: _capi.fim_plan_tokens_device(oo.data_ptr(), n_docs, n_ids, SEED, 0, 2**31, 2**31, True,
                                                            scratch.data_ptr(), plan.data_ptr(), kinds.data_ptr(), 0,
                                                            st.cuda_stream)}
        t = timed_alternating(fns, args.reps)
        packer.close()
    structure = n_docs * (8 + 2 * (8 + 32 + 4))
    moved = {"fim": n_ids * 4 + n_out * 8 + structure, "fim_all": n_ids * 4 + n_out * 20 + structure,
             "packed": n_ids * 4 + (n_docs + 1) * 8 + (n_ids // L + 1) * L * 12, "cut": n_docs * (8 + 24 + 4 + 6)}
    for k in fns:
        results[k] = summary(t[k])
        if k in moved:
            results[k]["bytes_moved"] = moved[k]
            results[k]["GBps"] = moved[k] / results[k]["median_ms"] / 1e6
    results["ratio_fim_all_over_torch"] = results["fim_all"]["median_ms"] / results["torch"]["median_ms"]
    results["ratio_fim_all_over_packed"] = results["fim_all"]["median_ms"] / results["packed"]["median_ms"]
    results["ratio_fim_over_packed"] = results["fim"]["median_ms"] / results["packed"]["median_ms"]
    results["faster_than_torch_beyond_its_spread"] = results["ratio_fim_all_over_torch"] < 1 - results["torch"]["spread"]
    print(json.dumps(results), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not results["faster_than_torch_beyond_its_spread"]:
        sys.exit("bench_fim: the HIP path is not faster than the torch composition by more than its spread")


if __name__ == "__main__":
    main()
