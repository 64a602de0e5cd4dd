#!/usr/bin/env python3
"""Token spans on the GPU (hutoken_amd.token_spans_device, csrc/hutk_spans.hip) against what a user of
encode_packed_device would write today, on one GPU in one process.

C3 (1 M documents) is encoded once per vocabulary through encode_packed_device -- VG (byte-level) and VL (characters,
prefix, ids of -1) -- then, per unit, three things are timed with device events, warmed up, alternating, `--reps` times:

  (a) new    the HIP path (int32 spans);
  (b) torch  torch_spans_* below: a gather of per-id lengths from a table, cumsum, minus each document's base, and a
             cumsum over the mask of character starts (or its nonzero()) plus gathers for the other unit -- the same
             tensor, asserted with torch.equal before anything is timed.  It trusts the ids; the HIP path also compares
             every token's bytes with the text;
  (c) copy   one torch.Tensor.copy_ that moves as many bytes as (a) reads plus writes (a copy of half that size);
  (d) search character mode only: the HIP path with HUTK_SPANS_SELECT=search, i.e. select by searching the counts of
             the rank structure instead of the scattered array (the other form of DESIGN 8b), asserted equal first.

Writes one JSON file (default profiles/spans_bench.json); fails without a GPU, and when (a) is not faster than (b) by more
than (b)'s spread.

  python tools/bench_spans.py [--docs N] [--reps R] [--out FILE] [--head NAME]
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


def token_tables(ctx, ids_used, n_table):
    """Per id (index id + 1; index 0 is the id -1): byte length and character count of its decoding, as a document's
    first token (prefix stripped) and elsewhere.  From the library's own decode of one- and two-token documents."""
    import numpy as np
    u = np.asarray(ids_used, dtype=np.int32)
    one, oo1, _ = ctx.decode_packed(u, np.arange(len(u) + 1, dtype=np.int64))
    two, oo2, _ = ctx.decode_packed(np.repeat(u, 2), 2 * np.arange(len(u) + 1, dtype=np.int64))
    tabs = np.zeros((4, n_table + 1), dtype=np.int64)  # len first, len rest, chars first, chars rest
    tabs[:, 0] = 1
    s1 = np.concatenate([[0], np.cumsum((one & 0xC0) != 0x80)])
    s2 = np.concatenate([[0], np.cumsum((two & 0xC0) != 0x80)])
    l1 = np.diff(oo1)
    tabs[0, u + 1] = l1
    tabs[1, u + 1] = np.diff(oo2) - l1
    tabs[2, u + 1] = s1[oo1[1:]] - s1[oo1[:-1]]
    tabs[3, u + 1] = (s2[oo2[1:]] - s2[oo2[:-1]]) - tabs[2, u + 1]
    return tabs


def _segments(ids, oo, n_ids, tab_first, tab_rest):
    """-> (units per token, running units inside the document after each token, document of each token)"""
    import torch
    dev = ids.device
    n_docs = oo.numel() - 1
    counts = oo[1:] - oo[:-1]
    j = torch.repeat_interleave(torch.arange(n_docs, device=dev), counts, output_size=n_ids)
    key = ids[:n_ids].long() + 1
    n = tab_rest[key]
    first = oo[:-1][counts > 0]
    n[first] = tab_first[key[first]]
    c = torch.cumsum(n, 0)
    base = (c - n)[oo[:-1].clamp(max=max(n_ids - 1, 0))]
    return n, c - base[j], j


def torch_spans_byte_mode(d_bytes, d_offs, ids, oo, n_ids, tabs, unit):
    import torch
    n, end, j = _segments(ids, oo, n_ids, tabs[0], tabs[1])
    start = end - n
    if unit == "byte":
        return torch.stack([start, end], 1).to(torch.int32)
    starts = torch.zeros(d_bytes.numel() + 1, dtype=torch.int64, device=d_bytes.device)
    torch.cumsum((d_bytes & 0xC0) != 0x80, 0, out=starts[1:])
    b = d_offs[:-1][j]
    s0 = starts[b]
    ce = starts[b + end] - s0
    cs = torch.where(n > 0, starts[(b + start + 1).clamp(max=d_bytes.numel())] - 1, starts[b + start]) - s0
    return torch.stack([cs, ce], 1).to(torch.int32)


def torch_spans_char_mode(d_bytes, d_offs, ids, oo, n_ids, tabs, unit):
    import torch
    n, end, j = _segments(ids, oo, n_ids, tabs[2], tabs[3])
    start = end - n
    if unit == "char":
        return torch.stack([start, end], 1).to(torch.int32)
    mask = (d_bytes & 0xC0) != 0x80
    sel = torch.cat([torch.nonzero(mask).flatten(), torch.tensor([d_bytes.numel()], device=d_bytes.device)])
    starts = torch.zeros(d_bytes.numel() + 1, dtype=torch.int64, device=d_bytes.device)
    torch.cumsum(mask, 0, out=starts[1:])
    b = d_offs[:-1][j]
    g = starts[b]
    return torch.stack([sel[g + start] - b, sel[g + end] - b], 1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spans_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_spans: no GPU; there is nothing to measure without one")
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
    d, o = synth.corpus("C3", args.docs)
    results = {"git_head": head, "device": torch.cuda.get_device_name(0), "corpus": "C3", "docs": args.docs,
               "bytes": int(o[-1]), "reps": args.reps, "configs": []}
    ok = True
    st = torch.cuda.Stream(dev)
    for vocab in ("VG", "VL"):
        vp, sp, kw = data.vocab_files(vocab)
        H.initialize(vp, sp, device=0, **kw)
        byte_mode = kw["is_byte_encoder"]
        with torch.cuda.stream(st):
            d_bytes, d_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
            ids, oo = H.encode_packed_device(d_bytes, d_offs)
            n_docs = oo.numel() - 1
            n_ids = int(oo[-1].item())
            n_chars = int(((d_bytes & 0xC0) != 0x80).sum().item())
            used = torch.unique(ids[:n_ids])
            used = used[used >= 0].cpu().numpy()
            tabs = torch.from_numpy(token_tables(H.context(), used, int(used.max()) + 1)).to(dev)
            unknown = int((ids[:n_ids] < 0).sum().item())
            ref = torch_spans_byte_mode if byte_mode else torch_spans_char_mode
            for unit in ("byte", "char"):
                label = "%s %s int32" % (vocab, unit)

                def new(unit=unit):
                    return H.token_spans_device(d_bytes, d_offs, ids, oo, unit=unit, n_ids=n_ids, check=False)

                def old(unit=unit):
                    return ref(d_bytes, d_offs, ids, oo, n_ids, tabs, unit)

                def search(unit=unit):
                    os.environ["HUTK_SPANS_SELECT"] = "search"  # (read by the library at every call)
                    try:
                        return new(unit)
                    finally:
                        del os.environ["HUTK_SPANS_SELECT"]

                got, want = H.token_spans_device(d_bytes, d_offs, ids, oo, unit=unit, n_ids=n_ids), old()
                torch.cuda.synchronize()
                assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), label
                if not byte_mode:
                    assert torch.equal(search(), want), label + " (search)"
                    torch.cuda.synchronize()
                del got, want
                # read: the ids, both offset arrays, the text twice (start bits, verification); written and read back:
                # the rank structure, in character mode the select array; written: the spans
                moved = n_ids * 4 + (n_docs + 1) * 16 + 2 * int(o[-1]) + 2 * (int(o[-1]) // 64) * 12 + n_ids * 8
                if not byte_mode:
                    moved += 2 * n_chars * 4
                half = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                other = torch.empty_like(half)
                fns = {"new": new, "torch": old, "copy": lambda: other.copy_(half)}
                if not byte_mode:
                    fns["search"] = search
                t = timed_alternating(fns, args.reps)
                del half, other
                r = {"config": label, "ids": n_ids, "unknown_ids": unknown, "bytes_moved": moved,
                     "new": summary(t["new"]), "torch": summary(t["torch"]), "copy": summary(t["copy"])}
                r["new_GBps"] = moved / r["new"]["median_ms"] / 1e6
                r["copy_GBps"] = moved / r["copy"]["median_ms"] / 1e6
                if not byte_mode:
                    r["search"] = summary(t["search"])
                    r["ratio_search_over_new"] = r["search"]["median_ms"] / r["new"]["median_ms"]
                r["ratio_new_over_torch"] = r["new"]["median_ms"] / r["torch"]["median_ms"]
                r["ratio_new_over_copy"] = r["new"]["median_ms"] / r["copy"]["median_ms"]
                r["faster_than_torch_beyond_its_spread"] = r["ratio_new_over_torch"] < 1 - r["torch"]["spread"]
                ok &= r["faster_than_torch_beyond_its_spread"]
                results["configs"].append(r)
                print(json.dumps(r), flush=True)
            del d_bytes, d_offs, ids, oo, tabs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not ok:
        sys.exit("bench_spans: the HIP path is not faster than the torch composition in every configuration")


if __name__ == "__main__":
    main()
