#!/usr/bin/env python3
"""Where the aggregation's time goes, and what the device replay changes.

Proves N chained synthetic 2^16-row segments on the GPU at the CLI options (the chain of
bench.py's multi-segment lines: program seed P, ops seed P + i, ROM lane 0 carried from segment
to segment), encodes the zl1 steps, then runs

  agg_prove(steps)            host replay, host ZlAggAir prover
  agg_prove(steps, ctx=ctx)   device replay, device ZlAggAir prover
  agg_prove(steps, ctx=ctx)   under agg_device_prover(0): device replay, host prover

alternately, `--reps` times each (the third only where the library has the switch), and the same
for verify_segments(proofs, ctx=ctx) against a loop of verify_segment.  Prints the medians, the
six agg_last_times() parts of every path (median per part, and every repetition) and whether the
artifacts / verdicts are equal, as one JSON object.  --package DIR takes the zkl_hip package from
another build (a worktree of another commit), for A/B runs of two builds by this one script.

One process, one context.  Run it under a time limit of its own, e.g.
  timeout -k 10 600 python scripts/agg_replay_time.py --children 64 --out profiles/agg_replay/n64.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM_SEED = 0x5EEDC400  # tests/golden/chain_2p16.json's program


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--children", type=int, default=64, help="segments in the chain (64 default, 256 the large case)")
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--verify-proofs", type=int, default=64, help="proofs in the verify_segments comparison (0: skip)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--package", default=os.path.join(ROOT, "zk-lisp_amd"),
                    help="directory holding the zkl_hip package to measure (default: this tree's)")
    ap.add_argument("--out", help="also write the JSON here")
    args = ap.parse_args()

    sys.path.insert(0, os.path.abspath(args.package))
    import zkl_hip
    n, N = 1 << args.log_n, args.children
    ctx = zkl_hip.Context(args.device)
    t0 = time.perf_counter()
    proofs, pis, opts, steps, rom0 = [], [], [], [], 0
    for i in range(N):
        trace, pi, w = zkl_hip.synth_vm_segment_chain(PROGRAM_SEED, PROGRAM_SEED + i, args.log_n, rom0)
        o = zkl_hip.proof_options(w, n)
        proof = ctx.prove_segment(trace, w, n, pi, o)
        info = zkl_hip.step_info_for(pi, i, N, i.to_bytes(32, "little"), (i + 1).to_bytes(32, "little"))
        steps.append(zkl_hip.step_proof_encode(pi, info, proof))
        proofs.append(proof), pis.append(pi), opts.append(o)
        rom0 = pi.rom_s_out[0].lo | (pi.rom_s_out[0].hi << 64)
    setup_s = time.perf_counter() - t0

    def timed(f):
        t = time.perf_counter()
        r = f()
        return (time.perf_counter() - t) * 1e3, r

    med = statistics.median
    res = {"children": N, "log_n": args.log_n, "reps": args.reps, "setup_s": round(setup_s, 1),
           "step_bytes": sum(len(s) for s in steps), "time_names": list(zkl_hip.AGG_TIME_NAMES)}

    # ---- aggregation: the paths alternately (one untimed call of each first)
    switch = getattr(zkl_hip, "agg_device_prover", None)
    paths = ["host", "device"] + (["device_host_prover"] if switch else [])
    res["package"] = os.path.relpath(os.path.abspath(args.package), ROOT)
    res["device_prover_switch"] = bool(switch)

    def run(path):
        if path == "host":
            return zkl_hip.agg_prove(steps)
        if path == "device" or not switch:
            return zkl_hip.agg_prove(steps, ctx=ctx)
        with switch(0):
            return zkl_hip.agg_prove(steps, ctx=ctx)

    want = run("host")
    equal = all(run(path) == want for path in paths[1:])
    ms = {path: [] for path in paths}
    parts = {path: [] for path in paths}
    for _ in range(args.reps):
        for path in paths:
            t, got = timed(lambda: run(path))
            equal = equal and got == want
            ms[path].append(t)
            parts[path].append(zkl_hip.agg_last_times())
    for path in paths:
        res[f"agg_{path}_ms"] = round(med(ms[path]), 2)
        res[f"agg_{path}_ms_all"] = [round(x, 2) for x in ms[path]]
        res[f"agg_{path}_parts_ms"] = [round(med(p[k] for p in parts[path]), 2) for k in range(6)]
        res[f"agg_{path}_parts_ms_all"] = [[round(x, 2) for x in p] for p in parts[path]]
    res["agg_artifacts_equal"] = equal

    # ---- verification: the batch on the device, the batch on host threads, a loop of verify_segment
    k = min(args.verify_proofs, N)
    if k:
        vp, vpi, vo = proofs[:k], pis[:k], opts[:k]

        def loop():
            out = []
            for p, pi, o in zip(vp, vpi, vo):
                try:
                    zkl_hip.verify_segment(p, pi, o)
                    out.append("")
                except zkl_hip.ZklError as e:
                    out.append(str(e))
            return out

        vwant = loop()
        vequal = zkl_hip.verify_segments(vp, vpi, vo, ctx=ctx) == vwant
        vms = {"loop": [], "batch_host": [], "batch_device": []}
        for _ in range(args.reps):
            t, got = timed(loop)
            vms["loop"].append(t)
            t, got = timed(lambda: zkl_hip.verify_segments(vp, vpi, vo))
            vequal = vequal and got == vwant
            vms["batch_host"].append(t)
            t, got = timed(lambda: zkl_hip.verify_segments(vp, vpi, vo, ctx=ctx))
            vequal = vequal and got == vwant
            vms["batch_device"].append(t)
        res["verify_proofs"] = k
        for name, v in vms.items():
            res[f"verify_{name}_ms"] = round(med(v), 2)
        res["verify_verdicts_equal"] = vequal
        res["verify_all_accept"] = vwant == [""] * k
    cur, peak = zkl_hip.pinned_bytes()
    res["pinned_bytes"] = {"current": cur, "peak": peak}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal and res.get("verify_verdicts_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
