#!/usr/bin/env python3
"""Row-aligned features on the GPU (hutoken_amd.gather_rows / token_word_ids_device / answer_positions and the row
planners, csrc/hutk_collate.hip and csrc/hutk_features.hip) kernel by kernel, against a copy of the same size and
against what a user of collate_windows writes without them; the method of tools/bench_collate.py.

C3 (1 M documents) is encoded once with VG under the gpt2 preset and cut into windows of 512 with stride 128 (eos).  Timed
with device events, 3 warm-up and `--reps` timed repetitions, the callables of one group alternating:

  planner        hutk_windows_plan_device on the row offsets of the windows
  gather spans   gather_rows of the int32 character spans (records of 8 bytes)          } each with `clone`, a torch.clone
  gather words   gather_rows of the int32 word ids (records of 4 bytes)                  } of a tensor the size of its
                                                                                           output (the copy floor), and
                                                                                           `torch`, the formulation below
  word ids       hutk_token_word_ids_device alone (bitmap, prefix counts and byte spans given), and token_word_ids_device
                 whole (the split, the count, the byte spans, the rank kernel)
  answers        answer_positions with one answer per document

The torch formulation is what a user writes today from row_map and lengths: an index rectangle, values[idx], torch.where
(asserted equal to gather_rows before anything is timed).  Bytes moved are computed from shapes.  Writes one JSON file
(default profiles/features_bench.json) with the ratios and whether the gap to torch lies outside the torch path's own
spread; no ratio is required.

  python tools/bench_features.py [--docs N] [--reps R] [--out FILE] [--head NAME]
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

EOS = 50256


def torch_gather(values, offs, row_map, lengths, L, fill):
    """The rows' rectangle of a per-token array from what collate_windows returns (eos only: ids begin at column 0)."""
    import torch
    col = torch.arange(L, device=values.device)[None, :]
    valid = col < (lengths - 1)[:, None]
    idx = ((offs[row_map[:, 0]] + row_map[:, 1])[:, None] + col).clamp_(0, values.shape[0] - 1)
    out = values[idx]
    if values.dim() == 2:
        valid = valid[:, :, None]
    return torch.where(valid, out, torch.tensor(fill, dtype=values.dtype, device=values.device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_features: no GPU; there is nothing to measure without one")
    import hutoken_amd as H
    from hutoken_amd import _capi, data, synth
    head = args.head
    if head is None:
        try:
            head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                           stderr=subprocess.DEVNULL).strip()
        except Exception:
            head = "unknown"
    dev = torch.device("cuda", 0)
    vp, sp, _kw = data.vocab_files("VG")
    H.initialize(vp, sp, is_byte_encoder=True, pretokenizer="gpt2")
    d, o = synth.corpus("C3", args.docs)
    L, stride = 512, 128
    st = torch.cuda.Stream(dev)  # a stream of torch's own: every call here is then ordered with the others
    results = {"git_head": head, "device": torch.cuda.get_device_name(0), "corpus": "C3", "vocab": "VG", "preset": "gpt2",
               "docs": args.docs, "bytes": int(o[-1]), "max_length": L, "stride": stride, "reps": args.reps, "warmup": 3,
               "kernels": []}

    def record(name, fns, moved, extra=None):
        t = timed_alternating(fns, args.reps)
        r = {"kernel": name, "bytes_moved": moved}
        r.update(extra or {})
        for k, ms in t.items():
            r[k] = summary(ms)
        r["new_GBps"] = moved / r["new"]["median_ms"] / 1e6
        if "clone" in r:
            r["ratio_new_over_clone"] = r["new"]["median_ms"] / r["clone"]["median_ms"]
        if "torch" in r:
            r["ratio_new_over_torch"] = r["new"]["median_ms"] / r["torch"]["median_ms"]
            r["gap_to_torch_outside_its_spread"] = abs(1 - r["ratio_new_over_torch"]) > r["torch"]["spread"]
        results["kernels"].append(r)
        print(json.dumps(r), flush=True)

    with torch.cuda.stream(st):
        d_bytes, d_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
        ids, oo = H.encode_packed_device(d_bytes, d_offs)
        n_docs, n_bytes, n_ids = args.docs, int(o[-1]), int(oo[-1].item())
        out, _mask, lengths, row_map, plan = H.collate_windows(ids, oo, L, stride, eos_id=EOS, n_ids=n_ids, return_plan=True, check=True)
        n_rows = out.shape[0]
        kept = int(lengths.sum().item()) - n_rows
        del out, _mask
        results.update({"ids": n_ids, "rows": n_rows, "ids_in_rows": kept})
        stream = torch.cuda.current_stream(dev).cuda_stream

        # the planner: reads offsets and row_offsets, writes 64 bytes a row
        row_offsets = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        _capi.windows_rows_device(oo.data_ptr(), n_docs, n_ids, L, stride, _capi.NO_TOKEN, EOS, row_offsets.data_ptr(), 0, stream)
        plan2 = torch.empty_like(plan)
        planner = lambda: _capi.windows_plan_device(oo.data_ptr(), row_offsets.data_ptr(), n_docs, n_ids, n_rows, L, stride,  # noqa: E731
                                                    _capi.NO_TOKEN, EOS, 0, plan2.data_ptr(), 0, stream)
        planner()
        assert torch.equal(plan, plan2)
        record("planner (windows)", {"new": planner}, n_rows * 64 + 2 * (n_docs + 1) * 8)

        # the gathers: rec bytes read per token column, rec bytes written per column, 64 bytes of plan per row
        spans = H.token_spans_device(d_bytes, d_offs, ids, oo, unit="char", n_ids=n_ids)
        words = H.token_word_ids_device(d_bytes, d_offs, ids, oo, n_ids=n_ids)
        for name, values, fill, rec in (("gather spans (rec 8)", spans, (0, 0), 8), ("gather word ids (rec 4)", words, -1, 4)):
            new = lambda: H.gather_rows(plan, L, values, fill=fill)  # noqa: E731
            ref = lambda: torch_gather(values, oo, row_map, lengths, L, fill[0] if rec == 8 else fill)  # noqa: E731
            got, want = new(), ref()
            assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), name
            del want
            record(name, {"new": new, "torch": ref, "clone": lambda: got.clone()}, kept * rec + n_rows * L * rec + n_rows * 64,
                   {"clone_bytes_moved": 2 * n_rows * L * rec})
            del got

        # the word-id kernel alone, and the whole call
        bits = H.pretokenize_packed_device(d_bytes, d_offs, "gpt2", return_bits=True)
        before = torch.zeros(n_bytes // 32 + 2, dtype=torch.int64, device=dev)
        H._pretokenizer(dev).starts_device(bits.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes, before.data_ptr(), 0, 0, stream)
        bspans = H.token_spans_device(d_bytes, d_offs, ids, oo, unit="byte", n_ids=n_ids)
        words2, status = torch.empty_like(words), torch.empty(n_docs, dtype=torch.int32, device=dev)
        kernel = lambda: _capi.token_word_ids_device(bits.data_ptr(), before.data_ptr(), d_offs.data_ptr(), n_docs, n_bytes,  # noqa: E731
                                                     bspans.data_ptr(), 4, oo.data_ptr(), n_ids, words2.data_ptr(),
                                                     status.data_ptr(), 0, stream)
        kernel()
        assert torch.equal(words, words2) and not bool(status.any())
        # read: a span, a bitmap word and a count per token (cached across neighbours), the id offsets; written: 4 bytes a token
        record("word ids (rank kernel)", {"new": kernel}, n_ids * 12 + n_bytes // 8 + n_bytes // 4 + 2 * (n_docs + 1) * 8 + n_docs * 4)
        record("word ids (whole call: split, count, byte spans, rank)",
               {"new": lambda: H.token_word_ids_device(d_bytes, d_offs, ids, oo, n_ids=n_ids, check=False)}, n_bytes + n_ids * 16)

        # answers: one answer of 8 characters per document
        chars = spans[(oo[1:] - 1).clamp_(min=0), 1].to(torch.int64) * (oo[1:] > oo[:-1])
        s = (chars // 3).to(torch.int32)
        answers = torch.stack([s, s + 8], dim=1).contiguous()
        new = lambda: H.answer_positions(plan, spans, answers, side="a")  # noqa: E731
        pos = new()
        results["rows_that_hold_their_answer"] = int((pos[:, 0] >= 0).sum().item())
        record("answers", {"new": new}, n_rows * (64 + 8 + 8) + n_rows * 2 * 10 * 8)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
