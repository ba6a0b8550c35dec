#!/usr/bin/env python3
"""Host traces as column pointers against one contiguous block, at the headline
segment (65,536 rows x 204 columns), one build per process.

The "trace table" of every pattern is W separately allocated columns that stay alive for the whole
run, as a Winterfell TraceTable holds them.

  a  the binding's pattern, per proof.  Without prove_segment_columns (the parent): a fresh
     contiguous allocation, the columns copied into it, prove_segment, the block freed.  With it:
     prove_segment_columns straight from the columns.
  b  prove_segment from one pageable block kept across proofs, with the upload loop's host time
     (and the staging statistics where the build has them).
  c  two contexts in flight on two threads, `--pairs` proofs each: proofs per second, pattern a.

Every pattern runs `--reps` times after one untimed run; medians and max - min are reported.
--package DIR takes the zkl_hip package from another build (a worktree of the parent commit): the
code under test is never its own baseline.  Prints one JSON object.

  timeout -k 10 300 python scripts/host_columns_time.py --out profiles/host_columns/this_1.json

--summarize PARENT.json THIS.json [...pairs] writes the comparison as markdown to stdout.  A gain
counts where this build's median is below the parent's by more than three times the parent's
max - min over all its runs of that pattern in the session.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stat(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "runs": len(xs)}


def measure(args):
    sys.path.insert(0, os.path.abspath(args.package))
    import zkl_hip
    tuning = zkl_hip.process_tuning(spin=True, malloc=False) if args.tuning else None
    n = 1 << args.log_n
    t, pi, w = zkl_hip.synth_vm_segment(0x5EED0001, args.log_n, 0)
    opts = zkl_hip.proof_options(w, n)
    mat = np.frombuffer(t, dtype=np.uint64).reshape(w, n * 2)
    cols = [np.array(mat[c]) for c in range(w)]  # one allocation per column
    ptrs = [int(c.ctypes.data) for c in cols]
    has_cols = hasattr(zkl_hip.Context, "prove_segment_columns")
    ctxs = [zkl_hip.Context(args.device) for _ in range(2)]
    ctx = ctxs[0]
    d = ctx.alloc(w * n * 16)
    ctx.upload(d, t, w * n * 16)
    want = ctx.prove_segment_device(d, w, n, pi, opts)
    ctx.free(d)

    def pattern_a(c, phases=None):
        t0 = time.perf_counter()
        if has_cols:
            proof = c.prove_segment_columns(ptrs, n, pi, opts)
            t1 = t2 = t0
            t3 = t4 = time.perf_counter()
        else:
            flat = np.empty((w, n * 2), dtype=np.uint64)  # fresh: first touch in the fill, unmapped on free
            t1 = time.perf_counter()
            for k in range(w):
                flat[k] = cols[k]
            t2 = time.perf_counter()
            proof = c.prove_segment(int(flat.ctypes.data), w, n, pi, opts)
            t3 = time.perf_counter()
            del flat
            t4 = time.perf_counter()
        if phases is not None:
            phases.append({"alloc": (t1 - t0) * 1e3, "fill": (t2 - t1) * 1e3, "call": (t3 - t2) * 1e3,
                           "free": (t4 - t3) * 1e3, "upload": c.host_times()["upload"]})
        if proof != want:
            raise RuntimeError("proof bytes differ from the device entry's")
        return (t4 - t0) * 1e3

    out = {"package": os.path.abspath(args.package), "has_columns_entry": has_cols, "log_n": args.log_n, "width": w,
           "reps": args.reps, "tuning": tuning}
    # a
    pattern_a(ctx)
    phases = []
    out["a_ms"] = stat([pattern_a(ctx, phases) for _ in range(args.reps)])
    out["a_phases_ms"] = {k: round(statistics.median(p[k] for p in phases), 3) for k in phases[0]}
    if has_cols:
        out["a_stats"] = ctx.upload_stats()
    # b
    block = np.array(mat)
    bp = int(block.ctypes.data)
    assert ctx.prove_segment(bp, w, n, pi, opts) == want
    calls, ups = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        ctx.prove_segment(bp, w, n, pi, opts)
        calls.append((time.perf_counter() - t0) * 1e3)
        ups.append(ctx.host_times()["upload"])
    out["b_call_ms"], out["b_upload_ms"] = stat(calls), stat(ups)
    if has_cols:
        out["b_stats"] = ctx.upload_stats()
    # c
    rates = []
    for rep in range(args.reps + 1):
        th = [threading.Thread(target=lambda c=c: [pattern_a(c) for _ in range(args.pairs)]) for c in ctxs]
        t0 = time.perf_counter()
        for x in th:
            x.start()
        for x in th:
            x.join()
        if rep:
            rates.append(2 * args.pairs / (time.perf_counter() - t0))
    out["c_proofs_per_s"] = stat(rates)
    for c in ctxs:
        c.close()
    return out


def summarize(paths):
    runs = [json.load(open(p)) for p in paths]
    par, new = runs[0::2], runs[1::2]
    print("| pattern | parent median (runs) | parent max - min | this build median (runs) | difference | bar (3 x spread) | claimed |")
    print("|---|---|---|---|---|---|---|")
    for key, unit, better in (("a_ms", "ms", -1), ("b_call_ms", "ms", -1), ("b_upload_ms", "ms", -1),
                              ("c_proofs_per_s", "proofs/s", 1)):
        pm = statistics.median(r[key]["median"] for r in par)
        nm = statistics.median(r[key]["median"] for r in new)
        spread = max(r[key]["max"] for r in par) - min(r[key]["min"] for r in par)
        gain = (nm - pm) * better
        print(f"| {key} ({unit}) | {pm:.2f} ({len(par)} x {par[0]['reps']}) | {spread:.2f} | {nm:.2f} ({len(new)} x "
              f"{new[0]['reps']}) | {nm - pm:+.2f} | {3 * spread:.2f} | "
              f"{'yes' if gain > 3 * spread else ('slower' if -gain > 3 * spread else 'no')} |")
    print()
    for name, rs in (("parent", par), ("this build", new)):
        ph = {k: statistics.median(r["a_phases_ms"][k] for r in rs) for k in rs[0]["a_phases_ms"]}
        print(f"- pattern a phases, {name} (ms, median): " + ", ".join(f"{k} {v:.2f}" for k, v in ph.items()))
    if "b_stats" in new[0]:
        print(f"- staging statistics, this build, pattern b: {new[0]['b_stats']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.join(ROOT, "zk-lisp_amd"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--tuning", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarize", nargs="+", default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    res = measure(args)
    txt = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
