#!/usr/bin/env python3
"""Training targets on the GPU (hutoken_amd.mask_tokens / lm_labels: k_rows_mlm and k_rows_labels of
csrc/hutk_collate.hip) against a copy of the same size and against what a user writes in torch today; the method of
tools/bench_features.py.

C3 (1 M documents) is encoded once with VG under the gpt2 preset and collated with an eos into padded rows of 512, into
windows of 512 with stride 128, and -- `dense`: all ids as ONE document in windows of 512 without stride -- into rows in
which every column but the eos is a token, where every column draws.  Timed with device events, 3 warm-up and `--reps`
timed repetitions, the callables of one group alternating:

  mlm tokens     mask_tokens in token mode        } each with `clone`, torch.clone of tensors the size of its outputs
  mlm words      mask_tokens in whole-word mode   } (the copy floor), and `torch`, the formulation below
  labels         lm_labels, loss on every real column
  labels shift   lm_labels with shift=True

The torch formulations are what a user writes today: the special-tokens mask rebuilt from lengths, bernoulli,
masked_fill, randint and three where calls for the corruption (whole words: a bernoulli per row and word, gathered by
the rows' word ids, which are given); where on the attention mask for the labels.  Before anything is timed the set of
eligible columns is asserted equal for the corruption (the random numbers cannot be) and the labels exactly.  Bytes moved
are computed from shapes.  Writes one JSON file (default profiles/targets_bench.json) with the ratios and whether the gap
to torch lies outside the torch path's own spread; no ratio is required.

  python tools/bench_targets.py [--docs N] [--reps R] [--out FILE] [--head NAME]
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

EOS, MASK_ID, VOCAB = 50256, 50257, 50257
P, P_MASK, P_RANDOM = 0.15, 0.8, 0.1


def torch_special(ids, lengths):
    """The special-tokens mask rebuilt from lengths (eos only, padded on the right: the ids are columns 0 .. length - 2)."""
    import torch
    col = torch.arange(ids.shape[1], device=ids.device)[None, :]
    return col >= (lengths - 1)[:, None]


def torch_corrupt(ids, selected):
    """DataCollatorForLanguageModeling.torch_mask_tokens behind the selection: 80 % mask, 10 % random, 10 % kept."""
    import torch
    labels = torch.where(selected, ids, -100)
    replaced = torch.bernoulli(torch.full(ids.shape, P_MASK, device=ids.device)).bool() & selected
    out = torch.where(replaced, MASK_ID, ids)
    random = torch.bernoulli(torch.full(ids.shape, P_RANDOM / (1 - P_MASK), device=ids.device)).bool() & selected & ~replaced
    words = torch.randint(VOCAB, ids.shape, dtype=ids.dtype, device=ids.device)
    return torch.where(random, words, out), labels


def torch_mlm(ids, lengths):
    import torch
    prob = torch.full(ids.shape, P, device=ids.device)
    prob.masked_fill_(torch_special(ids, lengths), 0.0)
    return torch_corrupt(ids, torch.bernoulli(prob).bool())


def torch_mlm_words(ids, lengths, word_rect, max_words):
    """A bernoulli per row and word, gathered by the rows' word ids (-1 on the special columns)."""
    import torch
    chosen = torch.bernoulli(torch.full((ids.shape[0], max_words), P, device=ids.device)).bool()
    selected = chosen.gather(1, word_rect.clamp(min=0).to(torch.int64)) & ~torch_special(ids, lengths)
    return torch_corrupt(ids, selected)


def torch_labels(ids, mask, shift):
    import torch
    real = mask.bool()
    if not shift:
        return torch.where(real, ids, -100)
    labels = torch.full_like(ids, -100)
    labels[:, :-1] = torch.where(real[:, :-1] & real[:, 1:], ids[:, 1:], -100)
    return labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_targets: no GPU; there is nothing to measure without one")
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
    vp, sp, _kw = data.vocab_files("VG")
    H.initialize(vp, sp, is_byte_encoder=True, pretokenizer="gpt2")
    d, o = synth.corpus("C3", args.docs)
    L, stride = 512, 128
    st = torch.cuda.Stream(dev)  # a stream of torch's own: every call here is then ordered with the others
    results = {"git_head": head, "device": torch.cuda.get_device_name(0), "corpus": "C3", "vocab": "VG", "preset": "gpt2",
               "docs": args.docs, "bytes": int(o[-1]), "max_length": L, "stride": stride, "reps": args.reps, "warmup": 3,
               "mlm_probability": P, "mask_fraction": P_MASK, "random_fraction": P_RANDOM, "layouts": []}

    def record(into, name, fns, moved, extra=None):
        t = timed_alternating(fns, args.reps)
        r = {"kernel": name, "bytes_moved": moved}
        r.update(extra or {})
        for k, ms in t.items():
            r[k] = summary(ms)
        r["new_GBps"] = moved / r["new"]["median_ms"] / 1e6
        r["ratio_new_over_clone"] = r["new"]["median_ms"] / r["clone"]["median_ms"]
        r["ratio_new_over_torch"] = r["new"]["median_ms"] / r["torch"]["median_ms"]
        r["gap_to_torch_outside_its_spread"] = abs(1 - r["ratio_new_over_torch"]) > r["torch"]["spread"]
        into.append(r)
        print(json.dumps(r), flush=True)

    with torch.cuda.stream(st):
        d_bytes, d_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
        ids, oo = H.encode_packed_device(d_bytes, d_offs)
        n_ids = int(oo[-1].item())
        words = H.token_word_ids_device(d_bytes, d_offs, ids, oo, n_ids=n_ids)
        results["ids"] = n_ids
        for layout in ("padded", "windows", "dense"):
            if layout == "padded":
                rows, mask, lengths, plan = H.collate_padded(ids, oo, L, eos_id=EOS, n_ids=n_ids, return_plan=True, check=True)
            elif layout == "dense":
                one = torch.tensor([0, n_ids], dtype=torch.int64, device=dev)
                rows, mask, lengths, _row_map, plan = H.collate_windows(ids, one, L, 0, eos_id=EOS, n_ids=n_ids, return_plan=True, check=True)
            else:
                rows, mask, lengths, _row_map, plan = H.collate_windows(ids, oo, L, stride, eos_id=EOS, n_ids=n_ids, return_plan=True,
                                                                        check=True)
            n_rows = rows.shape[0]
            kept = int(lengths.sum().item()) - n_rows  # eligible columns: every row has its eos
            rect = n_rows * L * 4
            word_rect = H.gather_rows(plan, L, words, fill=-1)
            max_words = int(word_rect.max().item()) + 1
            here = {"layout": layout, "rows": n_rows, "eligible_columns": kept, "fill": kept / (n_rows * L), "kernels": []}
            results["layouts"].append(here)
            special = torch_special(rows, lengths)
            for name, w, ref, extra_bytes in (("mlm tokens", None, lambda: torch_mlm(rows, lengths), 0),
                                              ("mlm words", words, lambda: torch_mlm_words(rows, lengths, word_rect, max_words), kept * 4)):
                kw = dict(mask_id=MASK_ID, vocab_size=VOCAB, mlm_probability=P, mask_fraction=P_MASK, random_fraction=P_RANDOM, word_ids=w)
                # what can be equal is: with probability 1 the selected columns are the eligible ones, torch's ~special
                _out, all_labels = H.mask_tokens(rows, plan, seed=1, **dict(kw, mlm_probability=1.0), check=True)
                assert torch.equal(all_labels != -100, ~special), name
                del _out, all_labels
                seeds = iter(range(2, 10**6))
                new = lambda: H.mask_tokens(rows, plan, seed=next(seeds), **kw)  # noqa: E731
                got, want = new(), ref()
                here.setdefault("selected_fraction", {})[name] = [float((x[1] != -100).sum().item()) / kept for x in (got, want)]
                del want
                record(here["kernels"], name, {"new": new, "torch": ref, "clone": lambda: (got[0].clone(), got[1].clone())},
                       3 * rect + n_rows * 64 + extra_bytes, {"clone_bytes_moved": 4 * rect})
                del got
            del special, word_rect
            for name, shift in (("labels", False), ("labels shift", True)):
                new = lambda: H.lm_labels(rows, mask, plan, shift=shift)  # noqa: E731
                ref = lambda: torch_labels(rows, mask, shift)  # noqa: E731
                got, want = new(), ref()
                assert got.dtype == want.dtype and torch.equal(got, want), name
                del want
                record(here["kernels"], name, {"new": new, "torch": ref, "clone": lambda: got.clone()},
                       2 * rect + n_rows * L + n_rows * 64, {"clone_bytes_moved": 2 * rect})
                del got
            del rows, mask, lengths, plan
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
