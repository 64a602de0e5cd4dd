#!/usr/bin/env python3
"""Throughput of the GPU normaliser (normalize_packed_device) on three corpora of hutoken_amd.synth:

  c3_clean      C3-shaped Hungarian, all clean under NFC (no table access, the write pass is a copy)
  c3_tenth_nfd  the same with every tenth document put through NFD on the host
  cjk           cjk_paragraphs: every character takes a table look-up

Per corpus and form: the sizes call, the write call, the full call with copy=True (sizes, one synchronising read, write),
the two calls enqueued back to back (n_out=: no read), and a device-to-device copy of the same bytes (torch.clone) as
the yardstick -- HIP events, warm-up, the median of the timed iterations -- and unicodedata.normalize over the list on
the host, once, for context.  Bars (clean corpus, NFC): sizes call <= copy, full call <= 2 x copy.

    python tools/measure_normalize.py --out profiles/normalize_throughput.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
import unicodedata

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(torch, fn, warmup, iters):
    """median milliseconds of fn() by HIP events on the current stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def tenth_nfd(data, offs):
    raw = data.tobytes()
    docs = [raw[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    for i in range(0, len(docs), 10):
        docs[i] = unicodedata.normalize("NFD", docs[i].decode("utf-8")).encode("utf-8")
    out = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, docs), dtype=np.int64, count=len(docs)), out=out[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000, help="documents of the C3 corpora")
    ap.add_argument("--cjk-docs", type=int, default=100000)
    ap.add_argument("--forms", default="NFC,NFKC")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out", default="profiles/normalize_throughput.json")
    args = ap.parse_args()
    import torch

    import hutoken_amd
    from hutoken_amd import _capi, synth
    if not torch.cuda.is_available():
        raise SystemExit("measure_normalize: no GPU; nothing is measured without one")
    tables = importlib.import_module("hutoken_amd.normalize")
    t0 = time.perf_counter()
    tables.table_blob()
    build_s = time.perf_counter() - t0
    dev = torch.device("cuda", 0)
    c3 = synth.corpus("C3", n_docs=args.docs)
    corpora = [("c3_clean", c3), ("c3_tenth_nfd", tenth_nfd(*c3)), ("cjk", synth.cjk_paragraphs(args.cjk_docs))]
    res = {"device": torch.cuda.get_device_name(0), "table_build_seconds": round(build_s, 3), "table_blob_bytes": len(tables.table_blob()),
           "chunk_bytes": _capi.norm_chunk_bytes(), "warmup": args.warmup, "iterations": args.iters, "statistic": "median, HIP events",
           "corpora": {}}
    for name, (data, offs) in corpora:
        db, do = torch.from_numpy(np.ascontiguousarray(data)).to(dev), torch.from_numpy(offs).to(dev)
        n_docs, n_bytes = len(offs) - 1, int(offs[-1])
        entry = {"docs": n_docs, "bytes": n_bytes, "forms": {}}
        entry["copy_ms"] = timed(torch, lambda: db.clone(), args.warmup, args.iters)
        raw = data.tobytes()
        texts = [raw[offs[i]:offs[i + 1]].decode("utf-8") for i in range(n_docs)]
        for form in args.forms.split(","):
            fi = tables.form_index(form)
            t0 = time.perf_counter()
            host = [unicodedata.normalize(form, t) for t in texts]
            host_s = time.perf_counter() - t0
            n_host_out = sum(len(t.encode("utf-8")) for t in host)
            del host
            nz = hutoken_amd._normalizer(dev)
            oo = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
            ch = torch.empty(n_docs, dtype=torch.uint8, device=dev)
            small = torch.zeros(4, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            text = (fi, db.data_ptr(), do.data_ptr(), n_docs, n_bytes)

            def sizes():
                nz.batch_device(*text, 0, 0, oo.data_ptr(), ch.data_ptr(), small.data_ptr(), small.data_ptr() + 16, stream)
            sizes()
            total, n_changed, err, _ = small.tolist()
            assert err == 0 and total == n_host_out, (name, form, err, total, n_host_out)
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)

            def write():
                nz.batch_device(*text, out.data_ptr(), total, 0, 0, 0, small.data_ptr() + 24, stream)
            f = {"out_bytes": total, "docs_changed": n_changed, "host_unicodedata_seconds": round(host_s, 3)}
            f["sizes_ms"] = timed(torch, sizes, args.warmup, args.iters)
            sizes()
            f["write_ms"] = timed(torch, write, args.warmup, args.iters)
            f["full_copy_true_ms"] = timed(torch, lambda: hutoken_amd.normalize_packed_device(db, do, form, copy=True), args.warmup, args.iters)
            f["enqueued_n_out_ms"] = timed(torch, lambda: hutoken_amd.normalize_packed_device(db, do, form, n_out=total), args.warmup, args.iters)
            for k in ("sizes_ms", "write_ms", "full_copy_true_ms", "enqueued_n_out_ms"):
                f[k.replace("_ms", "_over_copy")] = round(f[k] / entry["copy_ms"], 3)
                f[k.replace("_ms", "_GBps")] = round(n_bytes / f[k] / 1e6, 1)
            entry["forms"][form] = f
            print(name, form, json.dumps(f), flush=True)
        entry["copy_GBps_read_plus_write"] = round(2 * n_bytes / entry["copy_ms"] / 1e6, 1)
        res["corpora"][name] = entry
        del texts
    c = res["corpora"]["c3_clean"]
    nfc = c["forms"].get("NFC")
    if nfc:
        res["bars"] = {"sizes_call_at_most_copy": nfc["sizes_ms"] <= c["copy_ms"], "full_call_at_most_twice_copy": nfc["full_copy_true_ms"] <= 2 * c["copy_ms"],
                       "sizes_over_copy": nfc["sizes_over_copy"], "full_over_copy": nfc["full_copy_true_over_copy"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fobj:
        json.dump(res, fobj, indent=1)
        fobj.write("\n")
    print(json.dumps(res.get("bars")))


if __name__ == "__main__":
    main()
