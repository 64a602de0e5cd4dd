#!/usr/bin/env python3
"""Special tokens on the GPU (hutoken_amd.encode_special_packed_device, csrc/hutk_special.hip) against the plain encode
and against what a user does today, on one GPU in one process.

Corpus: C3 x VG, 1 M documents, in three forms:
  eot       "<|endoftext|>" appended to every document, the set {"<|endoftext|>": 50256}
  eot+256   the same text, the set with Llama-3's 256 "<|reserved_special_token_k|>" beside it (none occurs)
  plain     the unmodified corpus (zero matches): the price of asking when nothing is there
Candidates, timed with device events, warmed up, alternating inside every repetition:
  (a) special  encode_special_packed_device
  (b) plain    encode_packed_device on the same bytes: the parent's path, a lower bound, NOT a correct answer
  (c) host     today's way: re.split on the host, batch_encode of the text pieces, list stitching
(a) is asserted equal to (c) before anything is timed.  The kernels of (a) are then timed by groups (find, resolve, cut,
stitch; torch.profiler, one call) and put beside one torch.Tensor.copy_ of the bytes each group moves.

Writes one JSON file (default profiles/specials_bench.json); fails without a GPU, and when (a) is not faster than (c)
by more than (c)'s spread.

  python tools/bench_specials.py [--docs N] [--reps R] [--out FILE] [--head NAME]
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_collate import summary, timed_alternating  # noqa: E402

EOT = "<|endoftext|>"
GROUPS = {"find": ("k_sc_find",), "resolve": ("k_sc_resolve",), "cut": ("k_sc_count", "k_sc_write", "k_sc_docs"),
          "stitch": ("k_st_sum", "k_st_dst", "k_st_docs", "k_st_copy"), "scans": ("k_scan_i64",)}


def host_way(H, texts, specials, pattern):
    """re.split with a capturing group: text, marker, text, ..., text; the text pieces through batch_encode."""
    plans, pieces = [], []
    for t in texts:
        parts = pattern.split(t)
        plans.append(parts)
        pieces.extend(parts[0::2])
    enc = H.batch_encode(pieces)
    out, at = [], 0
    for parts in plans:
        row = []
        for k, p in enumerate(parts):
            if k & 1:
                row.append(specials[p])
            else:
                row.extend(enc[at])
                at += 1
        out.append(row)
    return out


def kernel_groups(fn):
    """One profiled call of fn -> {group: device microseconds}, or None when the profiler sees no kernels."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = dict.fromkeys(GROUPS, 0.0)
        seen = False
        for ev in prof.key_averages():
            us = getattr(ev, "device_time_total", None)
            if us is None:
                us = getattr(ev, "cuda_time_total", 0.0)
            for g, names in GROUPS.items():
                if any(n in ev.key for n in names):
                    out[g] += float(us)
                    seen = True
        return out if seen else None
    except Exception as e:  # no profiler in this build of torch: the groups are left out, the rest stands
        print("kernel groups not measured:", e)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specials_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_specials: no GPU; there is nothing to measure without one")
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
    raw = d.tobytes()
    plain_texts = [raw[int(o[i]):int(o[i + 1])].decode("utf-8") for i in range(args.docs)]
    eot_texts = [t + EOT for t in plain_texts]
    one = {EOT: 50256}
    many = dict(one, **{"<|reserved_special_token_%d|>" % k: 128002 + k for k in range(256)})
    results = {"git_head": head, "device": torch.cuda.get_device_name(0), "corpus": "C3", "vocab": "VG",
               "docs": args.docs, "reps": args.reps, "configs": []}
    ok = True
    st = torch.cuda.Stream(dev)
    for label, texts, specials in (("eot", eot_texts, one), ("eot+256", eot_texts, many), ("plain", plain_texts, one)):
        pattern = re.compile("(" + "|".join(re.escape(k) for k in sorted(specials, key=len, reverse=True)) + ")")
        H.set_special_tokens(specials)
        data_np, offs_np = H._pack(texts)
        with torch.cuda.stream(st):
            d_bytes, d_offs = torch.from_numpy(data_np.copy()).to(dev), torch.from_numpy(offs_np).to(dev)
            n_bytes, n_docs = d_bytes.numel(), d_offs.numel() - 1

            def special():
                return H.encode_special_packed_device(d_bytes, d_offs, check=False)

            def plain():
                return H.encode_packed_device(d_bytes, d_offs, check=False)

            def host():
                return host_way(H, texts, specials, pattern)

            ids, oo = H.encode_special_packed_device(d_bytes, d_offs)
            matches = H.context().special_last_matches
            want = host()
            want_oo = np.zeros(n_docs + 1, dtype=np.int64)
            np.cumsum([len(r) for r in want], out=want_oo[1:])
            want_ids = np.fromiter((x for r in want for x in r), dtype=np.int64, count=int(want_oo[-1])).astype(np.int32)
            assert np.array_equal(oo.cpu().numpy(), want_oo), label
            n_ids = int(want_oo[-1])
            assert np.array_equal(ids[:n_ids].cpu().numpy(), want_ids), label
            assert matches == (n_docs if label != "plain" else 0), (label, matches)
            del want, want_ids, ids, oo
            t = timed_alternating({"special": special, "plain": plain, "host": host}, args.reps)
            r = {"config": label, "bytes": n_bytes, "docs": n_docs, "specials": len(specials), "matches": matches,
                 "ids": n_ids, "special": summary(t["special"]), "plain": summary(t["plain"]), "host": summary(t["host"])}
            r["special_GBps"] = n_bytes / r["special"]["median_ms"] / 1e6
            r["plain_GBps"] = n_bytes / r["plain"]["median_ms"] / 1e6
            r["ratio_special_over_plain"] = r["special"]["median_ms"] / r["plain"]["median_ms"]
            r["ratio_special_over_host"] = r["special"]["median_ms"] / r["host"]["median_ms"]
            r["faster_than_host_beyond_its_spread"] = r["ratio_special_over_host"] < 1 - r["host"]["spread"]
            ok &= r["faster_than_host_beyond_its_spread"]
            groups = kernel_groups(special)
            if groups:
                n_pieces = n_docs + 2 * matches
                # bytes a group reads plus writes: the text and the length array; the length array; the selection twice
                # and the pieces' arrays; the pieces' arrays and the ids in and out
                moved = {"find": 2 * n_bytes, "resolve": n_bytes + 2 * matches,
                         "cut": 2 * n_bytes + 28 * matches + 16 * n_docs,
                         "stitch": 52 * n_pieces + 16 * n_docs + 8 * n_ids}
                r["kernel_groups"] = {}
                for g, us in groups.items():
                    e = {"kernels_ms": us / 1e3}
                    if g in moved and us > 0:
                        half = torch.empty(max(moved[g] // 2, 1), dtype=torch.uint8, device=dev)
                        other = torch.empty_like(half)
                        c = summary(timed_alternating({"copy": lambda: other.copy_(half)}, args.reps)["copy"])
                        e.update(bytes_moved=moved[g], copy_ms=c["median_ms"], ratio_over_copy=us / 1e3 / c["median_ms"])
                        del half, other
                    r["kernel_groups"][g] = e
            results["configs"].append(r)
            print(json.dumps(r), flush=True)
            del d_bytes, d_offs
            torch.cuda.empty_cache()
    H.set_special_tokens(None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        sys.exit("bench_specials: the device path is not faster than the host way beyond its spread in every configuration")


if __name__ == "__main__":
    main()
