#!/usr/bin/env python3
"""What the trace preflight costs next to the proof it guards.

For each shape (default: the headline 65,536 x 204 VM segment, and the 212-wide {vm, ram, rom}
segment of the rollup benchmark) a valid synthetic trace is made resident and

  ctx.check_trace_device(d_trace, w, n, pi)

is run `--reps` times: wall time of the call (kernel timing at its default), then again with
every kernel family timed (set_kernel_timing(2)), where kernel_times()["misc"] is the HIP-event
time around the check's launches (pose_k, the trace-domain evaluator instances, the assertion
kernel).  Next to the medians: stage_times() of one proof of the same trace on the same build
(CLI options), and the wall time of the CPU oracle's check of the same trace when the oracle
library is built (tests/oracle_lib.py).  Prints one JSON object; --out also writes it, --md
writes the table quoted in DESIGN.md.

One process, one context.  Run it under a time limit of its own, e.g.
  timeout -k 10 300 python scripts/preflight_time.py --out profiles/preflight/summary.json \\
      --md profiles/preflight/summary.md
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-lisp_amd"))

SHAPES = {"vm204": 0, "ram212": 2}  # name -> generator flags (zkl_synth_vm_segment_ex)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="vm204,ram212")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0001)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-oracle", action="store_true", help="skip the CPU oracle's check of the same trace")
    ap.add_argument("--out", help="also write the JSON here")
    ap.add_argument("--md", help="write the summary table here")
    args = ap.parse_args()

    import zkl_hip
    n = 1 << args.log_n
    ctx = zkl_hip.Context(args.device)
    med = statistics.median

    def timed(f):
        t = time.perf_counter()
        r = f()
        return (time.perf_counter() - t) * 1e3, r

    oracle = None
    if not args.no_oracle:
        try:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import oracle_lib
            oracle_lib.build()
            oracle = oracle_lib
        except Exception as e:  # noqa: BLE001  (the oracle is test infrastructure; the figures stand without it)
            print(f"# oracle unavailable: {e}", file=sys.stderr)

    res = {"log_n": args.log_n, "reps": args.reps, "shapes": {}}
    ok = True
    for name in args.shapes.split(","):
        flags = SHAPES[name]
        trace, pi, w = zkl_hip.synth_vm_segment(args.seed, args.log_n, flags)
        opts = zkl_hip.proof_options(w, n)
        nbytes = w * n * 16
        d = ctx.alloc(nbytes)
        ctx.upload(d, trace, nbytes)
        check = lambda: ctx.check_trace_device(d, w, n, pi)  # noqa: E731
        ok = ok and check() is None  # untimed: buffers, tables, code objects
        ctx.set_kernel_timing(1)
        wall = [timed(check)[0] for _ in range(args.reps)]
        ctx.set_kernel_timing(2)
        dev, wall_timed = [], []
        for _ in range(args.reps):
            t, rep = timed(check)
            ok = ok and rep is None
            wall_timed.append(t)
            dev.append(ctx.kernel_times()["misc"][0])
        ctx.prove_segment_device(d, w, n, pi, opts)  # untimed
        prove_ms, _ = timed(lambda: ctx.prove_segment_device(d, w, n, pi, opts))
        stages = {k: round(v, 3) for k, v in ctx.stage_times().items()}
        ctx.set_kernel_timing(1)
        host_wall = [timed(lambda: ctx.check_trace(trace, w, n, pi))[0] for _ in range(args.reps)]
        ctx.free(d)
        r = {"width": w, "n_rows": n, "check_device_ms": round(med(dev), 4), "check_device_ms_all": [round(x, 4) for x in dev],
             "check_wall_ms": round(med(wall), 3), "check_wall_ms_all": [round(x, 3) for x in wall],
             "check_wall_timed_ms": round(med(wall_timed), 3), "check_host_trace_wall_ms": round(med(host_wall), 3),
             "prove_wall_ms": round(prove_ms, 3), "stage_ms": stages}
        if oracle is not None:
            ot, opi, _ = oracle.synth_segment(args.seed, args.log_n, flags)
            t, got = timed(lambda: oracle.check_trace(ot, opi, w, n))
            ok = ok and got == (0, 0, 0)
            r["oracle_check_wall_ms"] = round(t, 1)
        res["shapes"][name] = r
    res["all_valid"] = ok
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(f"# Trace preflight, 2^{args.log_n} rows, median of {args.reps} (scripts/preflight_time.py)\n\n")
            f.write("| shape | check, device (ms) | check, call (ms) | host trace, call (ms) | evaluator stage (ms) | "
                    "proof, call (ms) | CPU oracle check (ms) |\n|---|---|---|---|---|---|---|\n")
            for name, r in res["shapes"].items():
                f.write(f"| {r['n_rows']} x {r['width']} ({name}) | {r['check_device_ms']} | {r['check_wall_ms']} | "
                        f"{r['check_host_trace_wall_ms']} | {r['stage_ms'].get('evaluator')} | {r['prove_wall_ms']} | "
                        f"{r.get('oracle_check_wall_ms', 'n/a')} |\n")
            f.write("\ncheck, device: HIP events around the check's launches (kernel timing mode 2); check, call: wall "
                    "time of check_trace_device at the default timing mode (host AIR instance, coefficient draws, "
                    "uploads, one round trip); host trace: check_trace, including the whole upload.\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
