#!/usr/bin/env python3
"""Best-fit packing (pack_best_fit) on one GPU in one process, in the manner of
tools/bench_packed.py: the same batch (C3, 1 M documents, encoded once with VG through encode_packed_device), device
events, 3 warm-up and `--reps` timed repetitions, the compared forms alternating, the outputs asserted equal before anything
is timed.  For seq_len 2048 and 8192:

  plan       hutk_bestfit_plan_device alone (rows_cap = the bound: no synchronisation), against the best host-side form
             this tool can write in numpy: the offsets copied down, the lengths' histogram, the same walk over groups of
             identical bins at count level (a Python loop over the length classes at most L / 2 long, the longer ones in
             numpy), the placements per visit in numpy, and the doc_map copied back up -- charged with both copies and
             the synchronisation they need
  rows       hutk_bestfit_rows_device alone, from a doc_map that lies on the device
  whole      pack_best_fit(n_ids=, n_rows=) with source, which never synchronises
  packer     for scale: SequencePacker.add + flush on the same batch
and beside the times the share of padding and the number of documents cut, for both packers.

Writes one JSON file (default profiles/bestfit_bench.json).

  python tools/bench_bestfit.py [--docs N] [--reps R] [--out FILE] [--head NAME] [--device-name NAME]
"""
import argparse
import bisect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_collate import summary, timed_alternating  # noqa: E402


def host_plan(offs, L, s):
    """offsets (numpy) -> doc_map int64 [n_docs, 4], (n_rows, W): the rule of include/hutoken_amd.h at count level.
    Groups of identical bins (first bin, bins, items so far) in one list per room, the rooms in use in a sorted list."""
    m = np.diff(offs) + s
    w, l = m // L, m % L
    n_docs = len(m)
    doc_map = np.full((n_docs, 4), -1, dtype=np.int64)
    first = np.cumsum(w) - w
    doc_map[:, 1] = w
    doc_map[:, 0] = np.where(w > 0, first, -1)
    W = int(w.sum())
    order = np.argsort(l, kind="stable")  # by class, document order inside a class
    hist = np.bincount(l, minlength=L)
    start = np.cumsum(hist) - hist
    # classes above L / 2: a bin per item, in numpy
    upper = np.arange(L - 1, L // 2, -1)
    upper = upper[hist[upper] > 0]
    bins = 0
    groups = {}   # room -> list of [first bin, bins, items so far], by first bin
    rooms = []    # the rooms that have groups, sorted
    if len(upper):
        firsts = np.cumsum(hist[upper]) - hist[upper]
        for cl, fb in zip(upper.tolist(), firsts.tolist()):
            docs = order[start[cl]:start[cl] + hist[cl]]
            doc_map[docs, 2] = W + fb + np.arange(hist[cl])
            doc_map[docs, 3] = 0
            groups[L - cl] = [[fb, int(hist[cl]), 1]]
        rooms = sorted(groups)
        bins = int(hist[upper].sum())

    def add(fb, n, room, items):
        if n <= 0 or room <= 0:
            return
        g = groups.get(room)
        if g is None:
            groups[room] = [[fb, n, items]]
            bisect.insort(rooms, room)
        else:
            bisect.insort(g, [fb, n, items])

    def place(docs, fb, k, room, cl):
        j = np.arange(len(docs))
        doc_map[docs, 2] = W + fb + j // k
        doc_map[docs, 3] = L - room + (j % k) * cl

    for cl in range(L // 2, 0, -1):
        c = int(hist[cl])
        if not c:
            continue
        docs = order[start[cl]:start[cl] + c]
        rank = 0
        while rank < c:
            at = bisect.bisect_left(rooms, cl)
            if at == len(rooms):
                break
            room = rooms[at]
            g = groups[room]
            fb, n, it = g[0]
            k = room // cl
            take = min(n * k, c - rank)
            place(docs[rank:rank + take], fb, k, room, cl)
            if take == n * k:
                g.pop(0)
                if not g:
                    del groups[room]
                    rooms.pop(at)
                add(fb, n, room - k * cl, it + k)
            else:
                n_full, t = take // k, take % k
                part = 1 if t else 0
                if n - n_full - part > 0:
                    g[0] = [fb + n_full + part, n - n_full - part, it]
                else:
                    g.pop(0)
                    if not g:
                        del groups[room]
                        rooms.pop(at)
                add(fb, n_full, room - k * cl, it + k)
                add(fb + n_full, part, room - t * cl, it + t)
            rank += take
        if rank < c:
            k = L // cl
            rem = c - rank
            place(docs[rank:], bins, k, L, cl)
            n_full, t = rem // k, rem % k
            part = 1 if t else 0
            add(bins, n_full, L - k * cl, k)
            add(bins + n_full, part, L - t * cl, t)
            bins += n_full + part
    return doc_map, (W + bins, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bestfit_bench.json"))
    ap.add_argument("--head", default=None, help="what to record as the git head (default: git rev-parse)")
    ap.add_argument("--device-name", default=None, help="the card's name for the record, where the driver reports a generic one")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_bestfit: no GPU; there is nothing to measure without one")
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
    vp, sp, kw = data.vocab_files("VG")
    H.initialize(vp, sp, device=0, **kw)
    d, o = synth.corpus("C3", args.docs)
    st = torch.cuda.Stream(dev)
    results = {"git_head": head, "device": args.device_name or torch.cuda.get_device_name(0),
               "arch": torch.cuda.get_device_properties(0).gcnArchName, "corpus": "C3", "vocab": "VG", "docs": args.docs,
               "bytes": int(o[-1]), "reps": args.reps, "configs": []}
    NO = _capi.NO_TOKEN
    with torch.cuda.stream(st):
        stream = st.cuda_stream
        d_bytes, d_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
        ids, oo = H.encode_packed_device(d_bytes, d_offs)
        n_ids = int(oo[-1].item())
        n_docs = oo.numel() - 1
        results["ids"] = n_ids
        lens = np.diff(oo.cpu().numpy())
        results["doc_ids_mean"] = float(lens.mean())
        results["doc_ids_max"] = int(lens.max())
        for L in (2048, 8192):
            s = 0
            bound = _capi.bestfit_rows_bound(n_docs, n_ids, L, s)
            doc_map = torch.empty((n_docs, 4), dtype=torch.int64, device=dev)
            info = torch.empty(2, dtype=torch.int64, device=dev)
            err = torch.zeros(2, dtype=torch.int32, device=dev)

            def plan():
                _capi.bestfit_plan_device(oo.data_ptr(), n_docs, n_ids, L, NO, NO, bound, doc_map.data_ptr(), info.data_ptr(),
                                          err.data_ptr(), stream)
                return doc_map

            host_map = torch.empty((n_docs, 4), dtype=torch.int64, device=dev)

            def host():
                dm, _info = host_plan(oo.cpu().numpy(), L, s)  # (the copy down synchronises)
                host_map.copy_(torch.from_numpy(dm), non_blocking=False)
                return host_map

            plan()
            host()
            torch.cuda.synchronize()
            n_rows, W = (int(x) for x in info.tolist())
            assert int(err[0]) == 0 and n_rows <= bound
            assert torch.equal(doc_map, host_map), "the device plan and the host plan differ"
            out = torch.empty((n_rows, L), dtype=torch.int32, device=dev)
            pos, seg = torch.empty_like(out), torch.empty_like(out)
            lengths = torch.empty(n_rows, dtype=torch.int32, device=dev)
            source = torch.empty((n_rows, L), dtype=torch.int64, device=dev)

            def rows():
                _capi.bestfit_rows_device(ids.data_ptr(), oo.data_ptr(), doc_map.data_ptr(), n_docs, n_ids, L, NO, NO, 0, 4, n_rows,
                                          out.data_ptr(), pos.data_ptr(), seg.data_ptr(), lengths.data_ptr(), source.data_ptr(),
                                          err[1:].data_ptr(), stream)
                return out

            def whole():
                return H.pack_best_fit(ids, oo, L, pad_id=0, n_ids=n_ids, n_rows=n_rows, return_source=True)

            packer = H.SequencePacker(L, pad_id=0)

            def packed():
                r = packer.add(ids, oo, n_ids=n_ids)
                packer.flush()
                return r

            rows()
            got = whole()
            torch.cuda.synchronize()
            assert int(err[1]) == 0
            for k, t in (("input_ids", out), ("position_ids", pos), ("segment_ids", seg), ("lengths", lengths), ("source", source)):
                assert torch.equal(got[k], t), k
            # what the rows are: every real element is its source's id, every document is there once
            real = source >= 0
            assert int(real.sum()) == n_ids and torch.equal(out[real], ids[:n_ids][source[real]])
            assert int(lengths.sum()) == n_ids and int((seg != 0).sum()) == n_ids
            del got, real
            t = timed_alternating({"plan": plan, "host_plan": host, "rows": rows, "whole": whole, "packer": packed}, args.reps)
            packer.close()
            m = lens + s
            begin = np.cumsum(m) - m
            packer_rows = -(-int(m.sum()) // L)
            r = {"config": "L=%d" % L, **{k: summary(v) for k, v in t.items()}, "n_rows": n_rows, "whole_rows": W,
                 "rows_bound": bound,
                 "best_fit_layout": {"rows": n_rows, "padding_share": 1 - n_ids / (n_rows * L), "documents_cut": int((m > L).sum())},
                 "packer_layout": {"rows": packer_rows, "padding_share": 1 - n_ids / (packer_rows * L),
                            "documents_cut": int(((m > 0) & (begin // L != (begin + m - 1) // L)).sum())}}
            r["ratio_plan_over_host_plan"] = r["plan"]["median_ms"] / r["host_plan"]["median_ms"]
            r["ratio_whole_over_packer"] = r["whole"]["median_ms"] / r["packer"]["median_ms"]
            r["rows_bytes_written"] = n_rows * L * 20 + n_rows * 4
            r["rows_GBps"] = r["rows_bytes_written"] / r["rows"]["median_ms"] / 1e6
            results["configs"].append(r)
            print(json.dumps(r), flush=True)
            del out, pos, seg, source

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
