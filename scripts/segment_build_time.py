#!/usr/bin/env python3
"""What building a segment's trace costs on the host and on the device.

Build times, median of `--reps`, one context:
  rollup-bench        tests/golden/programs.json, its one 65,536 x 212 segment
  fib-2pow16-log-n    tests/golden/programs.json, its whole trace (32,768 x 204: the program has
                      no 65,536-row segment)
  add-chain           a 2048-level Add chain (fib's op mix), one 65,536 x 204 segment
For each: the host builder on one thread into a pinned trace buffer (Program.segment_into); the
device build as HIP events around its upload and fill (kernel timing mode 2, build_device_ms); the
device build as call wall time, and call + synchronize; the host-trace upload loop of a proof of
the host-built trace (host_times()["upload"]); and the bytes the device build stages.  The device
trace is compared with the host one once per program.

Throughput: prove_program over the 16 segments of 65,536 rows of a 32,768-level Add chain with
inflight=4 (four contexts kept across the runs), CLI proof options: device_build=False at builders
1, 4, 8 (the code path of the commit before the device build, unchanged by it) and
device_build=True at builders=1, `--rounds` times in interleaved order; segments/s of each run and
the median.

One process.  Run it under a time limit of its own, e.g.
  timeout -k 10 500 python scripts/segment_build_time.py --out profiles/device_build/summary.json \\
      --md profiles/device_build/summary.md
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zk-lisp_amd"))


def add_chain(levels):
    from zkl_hip import op
    ops = [op("Const", dst=0, imm=1), op("Const", dst=1, imm=1)]
    ops += [op("Add", dst=k % 2, a=0, b=1) for k in range(levels - 3)]
    return ops + [op("End")]


def golden(name):
    import zkl_hip
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "programs.json")))[name]
    ops = [zkl_hip.op(k, **f) for k, f in g["ops"]]
    ma = [(tg, bytes.fromhex(b)) for tg, b in g["cli"]["main_args"]]
    return zkl_hip.Program(ops, bytes.fromhex(g["program_id"]), secret_args=g["cli"]["secret_u64"], main_args=ma), len(ops)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-throughput", action="store_true")
    ap.add_argument("--out", help="also write the JSON here")
    ap.add_argument("--md", help="write the summary table here")
    args = ap.parse_args()

    import ctypes as C
    import zkl_hip
    from zkl_hip.program import prove_program
    med = statistics.median
    pid = bytes(range(3, 35))

    def timed(f):
        t = time.perf_counter()
        r = f()
        return (time.perf_counter() - t) * 1e3, r

    programs = {"rollup-bench": golden("rollup-bench"), "fib-2pow16-log-n": golden("fib-2pow16-log-n")}
    ops = add_chain(2048)
    programs["add-chain"] = (zkl_hip.Program(ops, pid), len(ops))

    res = {"reps": args.reps, "build": {}, "throughput": {}}
    ok = True
    ctx = zkl_hip.Context(args.device)
    for name, (P, n_ops) in programs.items():
        a, b = zkl_hip.plan_segments(n_ops, 1 << 16)[0]
        m = b - a
        w = P.segment_width(a, b)
        nbytes = w * m * 16
        hbuf = ctx.trace_buffer(nbytes, 0)
        d = ctx.alloc(nbytes)
        pi, _, sin, sout = P.segment_into(a, b, hbuf)  # untimed: page faults of the pinned buffer
        got = ctx.build_segment_device(P, a, b, d, nbytes)  # untimed: buffers, code object
        same = ctx.download(d, nbytes) == C.string_at(hbuf, nbytes)
        same = same and (bytes(got[0]), got[1:]) == (bytes(pi), (w, sin, sout))
        ok = ok and same
        host = [timed(lambda: P.segment_into(a, b, hbuf))[0] for _ in range(args.reps)]
        inputs = [timed(lambda: P.segment_inputs(a, b))[0] for _ in range(args.reps)]
        ctx.set_kernel_timing(1)
        call, call_sync = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            ctx.build_segment_device(P, a, b, d, nbytes)
            t1 = time.perf_counter()
            ctx.synchronize()
            t2 = time.perf_counter()
            call.append((t1 - t0) * 1e3)
            call_sync.append((t2 - t0) * 1e3)
        ctx.set_kernel_timing(2)
        dev = []
        for _ in range(args.reps):
            ctx.build_segment_device(P, a, b, d, nbytes)
            dev.append(ctx.build_device_ms())
        ctx.set_kernel_timing(1)
        opts = zkl_hip.proof_options(w, m)
        ctx.prove_segment(hbuf, w, m, pi, opts)  # untimed
        up, prove_host, prove_dev = [], [], []
        for _ in range(args.reps):
            prove_host.append(timed(lambda: ctx.prove_segment(hbuf, w, m, pi, opts))[0])
            up.append(ctx.host_times()["upload"])
            prove_dev.append(timed(lambda: ctx.prove_segment_device(d, w, m, pi, opts))[0])
        ctx.free(d)
        r3 = lambda v: [round(x, 3) for x in v]  # noqa: E731
        res["build"][name] = {
            "width": w, "n_rows": m, "trace_bytes": nbytes, "equal_to_host": same,
            "host_build_ms": round(med(host), 3), "host_build_ms_all": r3(host),
            "segment_inputs_ms": round(med(inputs), 4),
            "device_build_event_ms": round(med(dev), 4), "device_build_event_ms_all": [round(x, 4) for x in dev],
            "device_build_call_ms": round(med(call), 3), "device_build_call_ms_all": r3(call),
            "device_build_call_sync_ms": round(med(call_sync), 3),
            "host_trace_upload_ms": round(med(up), 3), "host_trace_upload_ms_all": r3(up),
            "prove_host_trace_ms": round(med(prove_host), 3), "prove_device_trace_ms": round(med(prove_dev), 3)}
    ctx.close()

    if not args.no_throughput:
        ops = add_chain(16 * 2048)
        P = zkl_hip.Program(ops, pid)
        plan = zkl_hip.plan_segments(len(ops), 1 << 16)
        assert len(plan) == 16
        arms = [("host_builders_1", dict(builders=1)), ("host_builders_4", dict(builders=4)),
                ("host_builders_8", dict(builders=8)), ("device_builders_1", dict(builders=1, device_build=True))]
        runs = {k: [] for k, _ in arms}
        ctxs = [zkl_hip.Context(args.device) for _ in range(4)]  # kept: the runs time the segment loop alone
        proofs = {}
        for rnd in range(args.rounds + 1):  # round 0 untimed: code objects, allocator
            for k, kw in (arms if rnd % 2 else arms[::-1]):
                t, out = timed(lambda: prove_program(P, plan, contexts=ctxs, **kw))
                if rnd:
                    runs[k].append(len(plan) / (t / 1e3))
                    build = med([r.build_ms for r in out.values()])
                    res["throughput"].setdefault(k, {})["build_ms_median"] = round(build, 3)
                proofs.setdefault(k, [out[i].proof for i in sorted(out)])
        for c in ctxs:
            c.close()
        ok = ok and all(p == proofs["host_builders_1"] for p in proofs.values())
        for k, v in runs.items():
            res["throughput"][k].update({"segments_per_s": round(med(v), 2), "segments_per_s_all": [round(x, 2) for x in v]})
        res["throughput"]["shape"] = {"segments": 16, "n_rows": 1 << 16, "width": 204, "inflight": 4, "rounds": args.rounds}
    res["all_equal"] = ok
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write(f"# Segment trace build, host and device, median of {args.reps} (scripts/segment_build_time.py)\n\n")
            f.write("| program | rows x width | host build, 1 thread (ms) | device build, events (ms) | device build, "
                    "call (ms) | call + sync (ms) | host-trace upload (ms) | proof, host trace (ms) | proof, device "
                    "trace (ms) |\n|---|---|---|---|---|---|---|---|---|\n")
            for name, r in res["build"].items():
                f.write(f"| {name} | {r['n_rows']} x {r['width']} | {r['host_build_ms']} | {r['device_build_event_ms']} | "
                        f"{r['device_build_call_ms']} | {r['device_build_call_sync_ms']} | {r['host_trace_upload_ms']} | "
                        f"{r['prove_host_trace_ms']} | {r['prove_device_trace_ms']} |\n")
            f.write("\nhost build: zkl_build_segment_trace into a pinned trace buffer; device build, events: HIP events "
                    "around the staging upload and the fill; call: wall time of zkl_hip_build_segment_trace_device "
                    "(host staging, upload; the fill is only queued); host-trace upload: the upload loop of "
                    "zkl_hip_prove_segment on the host-built trace.\n")
            if res["throughput"]:
                t = res["throughput"]
                f.write(f"\n## prove_program, 16 segments of 65,536 x 204, inflight 4, median of {args.rounds} runs\n\n"
                        "| build | builders | segments/s | runs | build call, median (ms) |\n|---|---|---|---|---|\n")
                for k in ("host_builders_1", "host_builders_4", "host_builders_8", "device_builders_1"):
                    f.write(f"| {k.split('_')[0]} | {k.split('_')[-1]} | {t[k]['segments_per_s']} | "
                            f"{t[k]['segments_per_s_all']} | {t[k]['build_ms_median']} |\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
