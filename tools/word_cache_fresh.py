#!/usr/bin/env python3
"""What the word cache (csrc/hutk_wcache.h) is worth on documents it has NOT seen.  bench.py replays one batch, which
flatters a cache: every word of the timed steps was learned in the warm-up.  Here a context is warmed with the C3
documents [0, N) -- three batches, the table's entries after each -- and then encodes the documents [N, 2N) for the
first time (the "fresh pass"), then five times more (the replayed rate, for comparison).  The fresh pass is verified
against the oracle on its first 2000 documents.  The same is run for a context created under HUTK_WORD_CACHE=0.

    python tools/word_cache_fresh.py [--docs 1000000] [--log2 17 20 ...] [--vocab VG]

One JSON line per context: device times from the library's own events (hutk_last_timing: the tile kernel and the whole
enqueue), GB/s of input text over the whole enqueue."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--corpus", default="C3")
    ap.add_argument("--vocab", default="VG")
    ap.add_argument("--log2", type=int, nargs="*", default=[None], help="HUTK_WORD_CACHE_LOG2 values (default: the library's)")
    ap.add_argument("--no-off", action="store_true", help="skip the context without the table")
    args = ap.parse_args()

    import numpy as np
    import torch
    from hutoken_amd import _capi, data, synth
    from oracle import oracle as O
    O.build()
    dev = torch.device("cuda", 0)
    vp, sp, kw = data.vocab_files(args.vocab)
    orc = O.Oracle(vp, sp, kw["prefix"], kw["is_byte_encoder"])
    warm = synth.corpus(args.corpus, args.docs)
    fresh = synth.corpus(args.corpus, args.docs, first_doc=args.docs)
    n_check = min(2000, args.docs)
    want_ids, want_oo, _ = orc.encode_packed(fresh[0][:int(fresh[1][n_check])], fresh[1][:n_check + 1], 8)

    def on_device(d, o):
        nb = int(o[-1])
        return (torch.from_numpy(np.array(d[:nb], dtype=np.uint8, copy=True)).to(dev), torch.from_numpy(np.ascontiguousarray(o)).to(dev),
                len(o) - 1, nb)

    batches = {"warm": on_device(*warm), "fresh": on_device(*fresh)}
    stream = torch.cuda.Stream(dev)

    def run(ctx, which):
        db, do, n, nb = batches[which]
        cap = ctx.ids_capacity(nb, n)
        ids = torch.empty(cap, dtype=torch.int32, device=dev)
        oo = torch.empty(n + 1, dtype=torch.int64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        ctx.encode_device(db.data_ptr(), do.data_ptr(), n, nb, ids.data_ptr(), cap, oo.data_ptr(), 0, err.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert int(err.item()) == 0
        k_ms, all_ms = ctx.last_timing()
        return {"k_tiles_ms": round(k_ms, 4), "ms": round(all_ms, 4), "GB/s": round(nb / all_ms / 1e6, 1)}, ids, oo

    settings = ([] if args.no_off else ["off"]) + list(args.log2)
    for setting in settings:
        env = {"HUTK_WORD_CACHE": "0"} if setting == "off" else {} if setting is None else {"HUTK_WORD_CACHE_LOG2": str(setting)}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"], device=0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        out = {"table": setting if setting is not None else "default", "docs": args.docs, "corpus": args.corpus, "vocab": args.vocab,
               "warm_bytes": batches["warm"][3], "fresh_bytes": batches["fresh"][3], "warmup": []}
        for i in range(3):  # (the first of them is the cold cost: a fresh context's first batch)
            r, _, _ = run(ctx, "warm")
            r.update(ctx.word_cache_stats())
            out["warmup"].append(r)
        rep = [run(ctx, "warm")[0] for _ in range(5)]
        out["warm_replayed_mean"] = {k: round(sum(x[k] for x in rep) / len(rep), 4) for k in rep[0]}
        r, ids, oo = run(ctx, "fresh")
        st = ctx.word_cache_stats()
        r.update(appended=st["appended"], entries=st["entries"], open=st["open"])
        out["fresh_pass"] = r
        oo_h = oo[:n_check + 1].cpu().numpy()
        ids_h = ids[:int(oo_h[-1])].cpu().numpy()
        out["fresh_pass_equals_oracle_on_docs"] = n_check if np.array_equal(oo_h, want_oo) and np.array_equal(ids_h, want_ids) else -1
        rep = [run(ctx, "fresh")[0] for _ in range(5)]
        out["fresh_replayed_mean"] = {k: round(sum(x[k] for x in rep) / len(rep), 4) for k in rep[0]}
        out["stats_end"] = ctx.word_cache_stats()
        print(json.dumps(out), flush=True)
        assert out["fresh_pass_equals_oracle_on_docs"] == n_check, "the fresh pass differs from the oracle"
        ctx.close()


if __name__ == "__main__":
    main()
