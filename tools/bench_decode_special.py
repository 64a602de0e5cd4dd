#!/usr/bin/env python3
"""Decoding with special ids, device-resident, by the method of tools/bench_decode.py --events: device events around every
call, 3 warm-up and 20 timed repetitions, the variants ALTERNATING inside a repetition; medians and (max - min) / median.

Workload: the ids of C3 x VG, 1 M documents, from hutk_encode_special_batch_device with "<|endoftext|>" (id 50256) appended
to every document.  Timed:
  (a) hutk_decode_special_batch_device, flags 0          -> the text, markers included
  (b) the same with HUTK_DECODE_SKIP_SPECIAL             -> the text without them
  (c) hutk_decode_batch_device on the same ids           (the marker is vocabulary line 50256 of VG, so it runs)
Every variant's output is compared with the text it must give before anything is timed.

--parent-lib PATH: a build of the parent commit's library.  (c) is then also run in processes of their own, parent, this
tree, parent, this tree, on the card of this process: the plain path must stay within the parent's own run-to-run spread
(profiles/decode_special_isa_identity.txt says why it should).  --plain-only is what those processes run.
Writes --out (profiles/decode_special_bench.json) and prints it."""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_special_bench.json"))
args = ap.parse_args()

import numpy as np, torch
from hutoken_amd import _capi, data, synth

EOT, EOT_ID = b"<|endoftext|>", 50256
vp, sp, kw = data.vocab_files("VG")
ctx = _capi.Context(vp, sp, kw["prefix"], kw["is_byte_encoder"])
ctx.set_special_tokens([(EOT, EOT_ID)])
d, o = synth.corpus("C3", args.docs)
n = args.docs
# every document with the marker behind it
lens = np.diff(o)
o2 = o + len(EOT) * np.arange(n + 1, dtype=np.int64)
d2 = np.empty(int(o2[-1]), dtype=np.uint8)
d2[np.arange(len(d), dtype=np.int64) + len(EOT) * np.repeat(np.arange(n, dtype=np.int64), lens)] = d
d2[(o2[1:, None] - len(EOT) + np.arange(len(EOT), dtype=np.int64)[None, :]).ravel()] = np.tile(np.frombuffer(EOT, np.uint8), n)

dev = torch.device("cuda", 0)
db, do = torch.from_numpy(d2).to(dev), torch.from_numpy(o2).to(dev)
plain_text, plain_offs = torch.from_numpy(d).to(dev), torch.from_numpy(o).to(dev)
cap = ctx.special_ids_capacity(len(d2), n)
ids = torch.empty(cap, dtype=torch.int32, device=dev)
oo = torch.empty(n + 1, dtype=torch.int64, device=dev)
err = torch.zeros(1, dtype=torch.int32, device=dev)
# a stream of this tool's own: the C ABI reads torch's NULL stream as "the context's stream", which the events of the NULL
# stream would not wait for
side = torch.cuda.Stream(dev)
torch.cuda.synchronize()
torch.cuda.set_stream(side)
st = side.cuda_stream
assert st != 0
ctx.encode_special_device(db.data_ptr(), do.data_ptr(), n, len(d2), ids.data_ptr(), cap, oo.data_ptr(), 0, err.data_ptr(), st)
torch.cuda.synchronize()
assert int(err.item()) == 0 and ctx.special_last_matches == n
n_ids = int(oo[-1])
ids = ids[:n_ids].clone()
text = torch.empty(len(d2) + 64, dtype=torch.uint8, device=dev)
boff = torch.empty(n + 1, dtype=torch.int64, device=dev)


def special(flags):
    ctx.decode_special_device(ids.data_ptr(), oo.data_ptr(), n, n_ids, flags, text.data_ptr(), len(d2) + 64, boff.data_ptr(), 0,
                              err.data_ptr(), st)


def plain():
    ctx.decode_device(ids.data_ptr(), oo.data_ptr(), n, n_ids, text.data_ptr(), len(d2) + 64, boff.data_ptr(), 0, err.data_ptr(), st)


variants = {"plain": (plain, db, do)} if args.plain_only else {
    "special": (lambda: special(0), db, do), "special_skip": (lambda: special(_capi.DECODE_SKIP_SPECIAL), plain_text, plain_offs),
    "plain": (plain, db, do)}
for name, (fn, want, want_offs) in variants.items():
    fn()
    torch.cuda.synchronize()
    assert int(err.item()) == 0, name
    assert torch.equal(boff, want_offs) and torch.equal(text[:want.numel()], want), name + ": not the text"

times = {name: [] for name in variants}
for rep in range(args.warmup + args.steps):
    evs = []
    for name, (fn, _w, _o) in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        fn()
        b.record(side)
        evs.append((name, a, b))
    torch.cuda.synchronize()
    if rep >= args.warmup:
        for name, a, b in evs:
            times[name].append(a.elapsed_time(b))


def summary(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
            "spread": round((ms[-1] - ms[0]) / med, 4)}


result = {"workload": f"C3 x VG, {n} documents, '<|endoftext|>' behind each: {len(d2) / 1e6:.1f} MB of text, {n_ids} ids, "
                      "device-resident", "steps": args.steps, "warmup": args.warmup,
          "library": os.environ.get("HUTOKEN_AMD_LIB") or "this tree", "device": torch.cuda.get_device_name(0),
          **{name: summary(ms) for name, ms in times.items()}}
for name in times:
    out_bytes = len(d) if name == "special_skip" else len(d2)
    result[name]["GB_per_s_of_text"] = round(out_bytes / result[name]["ms_median"] / 1e6, 2)
if args.plain_only:
    print(json.dumps(result))
    sys.exit(0)

if args.parent_lib:
    runs = []
    for which in ("parent", "this tree", "parent", "this tree"):
        env = dict(os.environ)
        env.pop("HUTOKEN_AMD_LIB", None)
        if which == "parent":
            env["HUTOKEN_AMD_LIB"] = os.path.abspath(args.parent_lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--docs", str(args.docs), "--steps",
                            str(args.steps), "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=600)
        if p.returncode:
            sys.stderr.write(p.stderr)
            sys.exit("the plain-only run of %s failed (exit status %d); nothing more is started" % (which, p.returncode))
        r = json.loads(p.stdout.strip().splitlines()[-1])
        runs.append({"library": which, **r["plain"]})
    result["plain_parent_vs_head"] = runs
    par = [r["ms_median"] for r in runs if r["library"] == "parent"]
    head = [r["ms_median"] for r in runs if r["library"] == "this tree"]
    result["plain_parent_run_to_run"] = round(abs(par[0] - par[1]) / min(par), 4)
    result["plain_head_over_parent"] = round((sum(head) / 2) / (sum(par) / 2), 4)
a, c = result["special"]["ms_median"], result["plain"]["ms_median"]
result["special_over_plain"] = round(a / c, 4)
result["skip_over_plain"] = round(result["special_skip"]["ms_median"] / c, 4)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
