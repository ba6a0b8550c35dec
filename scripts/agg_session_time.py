#!/usr/bin/env python3
"""The tail after the last segment proof: aggregation at the end against an aggregation session
that replays each step proof while the others prove.

The children are the first N segments (65,536 rows each) of examples/fib-2pow16.zlisp, proved at
the CLI options by prove_program with `--inflight` contexts; the aggregation runs on a context of
its own.

  path a   prove_program, steps_of, then agg_prove(steps, ctx=...): the tail is that call's
           slot [5] of agg_last_times()
  path b   prove_chain: the tail is its tail_ms, from the return of the last segment proof to
           the return of the session's finish (only where the package has prove_chain)

The paths alternate, `--reps` times each after one untimed run of each, in one process; segments
per second are N over the wall time of the whole run of a path.  Prints one JSON object.
--package DIR takes the zkl_hip package from another build (a worktree of the parent commit),
which supplies path a and its spread: the code under test is never its own baseline.

  timeout -k 10 600 python scripts/agg_session_time.py --children 64 --out profiles/agg_session/this_n64.json

--summarize PARENT.json THIS.json [...pairs] writes the comparison as markdown to stdout: the change
counts where path b's tail is below the parent's path a by more than three times the parent's
max - min over its repetitions, and the proofs count as not slowed where path b's segments per
second are not below the parent's by more than three times its spread.
"""
import argparse
import gzip
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIB = os.path.join(ROOT, "tests", "golden", "fib_2pow16.json")


def load_fib(zkl_hip):
    g = json.load(open(FIB))
    raw = gzip.open(os.path.join(os.path.dirname(FIB), g["ops_file"])).read()
    if hashlib.sha256(raw).hexdigest() != g["ops_json_sha256"]:
        raise RuntimeError("fib-2pow16 op list fixture does not match its sha256")
    ops = [zkl_hip.op(k, **f) for k, f in json.loads(raw)]
    return ops, bytes.fromhex(g["program_id"]), g["max_segment_rows"]


def measure(args):
    sys.path.insert(0, os.path.abspath(args.package))
    import zkl_hip
    from zkl_hip import program
    tuning = zkl_hip.process_tuning(spin=True, malloc=True) if args.tuning else None  # as bench.py does
    ops, pid, max_rows = load_fib(zkl_hip)
    P = zkl_hip.Program(ops, pid)
    plan = zkl_hip.plan_segments(len(ops), max_rows)[:args.children]
    N = len(plan)
    ctxs = [zkl_hip.Context(args.device) for _ in range(args.inflight)]
    actx = zkl_hip.Context(args.device)
    kw = dict(contexts=ctxs, builders=args.builders, device_build=bool(args.device_build))
    has_chain = hasattr(program, "prove_chain")
    paths = ["a"] + (["b"] if has_chain else [])

    def run(path):
        """(artifact, tail ms, whole wall s, the six aggregation times)"""
        t0 = time.perf_counter()
        if path == "a":
            recs = program.prove_program(P, plan, **kw)
            steps = program.steps_of(recs.values(), N)
            art, _ = zkl_hip.agg_prove(steps, ctx=actx)
            times = zkl_hip.agg_last_times()
            return art, times[5], time.perf_counter() - t0, times
        r = program.prove_chain(P, plan, agg_ctx=actx, **kw)
        return r["artifact"], r["tail_ms"], time.perf_counter() - t0, r["times"]

    res = {"package": os.path.relpath(os.path.abspath(args.package), ROOT), "children": N, "rows": max_rows,
           "reps": args.reps, "inflight": args.inflight, "builders": args.builders,
           "device_build": bool(args.device_build), "process_tuning": tuning, "paths": paths,
           "time_names": list(zkl_hip.AGG_TIME_NAMES)}
    want = None
    equal = True
    for path in paths:  # warm every shape: code objects, context buffers, the aggregation context
        art = run(path)[0]
        want = want or art
        equal = equal and art == want
    out = {p: {"tail_ms": [], "seg_per_s": [], "parts_ms": []} for p in paths}
    for _ in range(args.reps):
        for path in paths:
            art, tail, wall, parts = run(path)
            equal = equal and art == want
            out[path]["tail_ms"].append(round(tail, 2))
            out[path]["seg_per_s"].append(round(N / wall, 3))
            out[path]["parts_ms"].append([round(x, 2) for x in parts])
    for path in paths:
        o = out[path]
        o["tail_ms_median"] = round(statistics.median(o["tail_ms"]), 2)
        o["tail_ms_spread"] = round(max(o["tail_ms"]) - min(o["tail_ms"]), 2)
        o["seg_per_s_median"] = round(statistics.median(o["seg_per_s"]), 3)
        o["seg_per_s_spread"] = round(max(o["seg_per_s"]) - min(o["seg_per_s"]), 3)
        o["parts_ms_median"] = [round(statistics.median(p[k] for p in o["parts_ms"]), 2) for k in range(6)]
        res["path_" + path] = o
    res["artifacts_equal"] = equal
    res["artifact_sha256"] = hashlib.sha256(want).hexdigest()
    zkl_hip.agg_verify(want)
    for c in ctxs + [actx]:
        c.close()
    P.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


def summarize(files):
    if len(files) % 2:
        raise SystemExit("--summarize takes pairs: PARENT.json THIS.json")
    rows, verdicts = [], []
    for k in range(0, len(files), 2):
        par, this = (json.loads(open(f).read()) for f in files[k:k + 2])
        n = par["children"]
        pa, ta, tb = par["path_a"], this["path_a"], this["path_b"]
        for name, o in (("parent, a: aggregation at the end", pa), ("this, a: aggregation at the end", ta),
                        ("this, b: prove_chain", tb)):
            rows.append("| %d | %s | %.2f | %.2f | %.2f | %.2f | %s |" % (
                n, name, o["tail_ms_median"], o["tail_ms_spread"], o["seg_per_s_median"], o["seg_per_s_spread"],
                " / ".join("%.1f" % x for x in o["parts_ms_median"])))
        bar_t, bar_r = 3 * pa["tail_ms_spread"], 3 * pa["seg_per_s_spread"]
        gain = pa["tail_ms_median"] - tb["tail_ms_median"]
        loss = pa["seg_per_s_median"] - tb["seg_per_s_median"]
        same = par["artifact_sha256"] == this["artifact_sha256"] and par["artifacts_equal"] and this["artifacts_equal"]
        verdicts.append("| %d | %.2f | %.2f | %.2f | %+.2f | %s | %.3f | %.3f | %+.3f | %s | %s |" % (
            n, pa["tail_ms_median"], bar_t, tb["tail_ms_median"], -gain, "yes" if gain > bar_t else "no",
            pa["seg_per_s_median"], bar_r, -loss, "yes" if loss <= bar_r else "no", "yes" if same else "NO"))
    print("| children | build, path | tail ms (median) | tail spread | segments/s (median) | segments/s spread | "
          "times [0..5] ms |")
    print("|---|---|---|---|---|---|---|")
    print("\n".join(rows))
    print()
    print("| children | parent tail | bar (3 x spread) | prove_chain tail | change | tail counts | parent segments/s | "
          "bar (3 x spread) | change | no loss beyond the bar | same artifact |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    print("\n".join(verdicts))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--children", type=int, default=64, help="segments of fib-2pow16 to prove and aggregate (64, 256)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--builders", type=int, default=8)
    ap.add_argument("--device-build", type=int, default=1,
                    help="1: traces built on the device (default), 0: host builders")
    ap.add_argument("--tuning", type=int, default=1,
                    help="1: zkl_hip.process_tuning(spin, malloc) first, as bench.py applies it (default); 0: none")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--package", default=os.path.join(ROOT, "zk-lisp_amd"),
                    help="directory holding the zkl_hip package to measure (default: this tree's)")
    ap.add_argument("--out", help="also write the JSON here")
    ap.add_argument("--summarize", nargs="+", metavar="JSON", help="PARENT.json THIS.json pairs -> markdown tables")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    return measure(args)


if __name__ == "__main__":
    sys.exit(main())
