"""`zk-lisp prove`'s segment loop on one device (prove.rs:1000-1175): every segment of a program
built by the per-segment builder (no full trace) and proved by `inflight` contexts -- the
reference's bounded rayon pool (prove.rs:1018-1050) -- and wrapped as zl1 step proofs.

By default a segment is built on a host thread (zkl_build_segment_trace) straight into a context's
pinned trace buffer (zkl_hip_trace_buffer) and proved through the host-trace entry point
(zkl_hip_prove_segment: the columns DMA'd from that buffer, overlapped with their LDE).  Per
context the next segment is built into the second buffer slot while the current one proves, so
host building (~0.2 s per 65,536-row segment on one thread, which is why `builders` defaults to 8)
overlaps the GPU.

With device_build=True the trace is written on the device instead
(zkl_hip_build_segment_trace_device): the host stages a few hundred bytes per level
and the context fills one of its two device trace buffers, proved with prove_segment_device.
"""
from __future__ import annotations

import threading
import time
from concurrent.futures import ThreadPoolExecutor, wait

from . import AGG_TRACE_VALID, AggSession, Context, Program, ZklError, proof_options, step_info_for, step_proof_encode


class SegmentProof:
    __slots__ = ("index", "rows", "width", "pi", "state_in", "state_out", "opts", "proof", "build_ms", "prove_ms")

    def __init__(self, index, rows, width, pi, state_in, state_out, opts):
        self.index, self.rows, self.width, self.pi = index, rows, width, pi
        self.state_in, self.state_out, self.opts = state_in, state_out, opts
        self.proof = None
        self.build_ms = self.prove_ms = 0.0


def prove_program(program: Program, plan, device: int = 0, inflight: int = 4, builders: int = 8, segments=None,
                  queries: int = 64, blowup: int = 16, grind: int = 16, contexts=None, on_proof=None,
                  preflight: bool = False, device_build: bool = False):
    """Proves the segments of `plan` ([(r_start, r_end)], zkl_plan_segments) whose indices are in
    `segments` (default all): returns {index: SegmentProof}.  `contexts` may pass existing
    Contexts (then `inflight` = their count and they stay open).  on_proof(SegmentProof) runs in
    the proving thread after each proof.  preflight=True checks every segment's trace on the device
    before its proof (Context.set_preflight, on the contexts created here): a trace that violates the
    AIR raises ZklError naming the constraint and row instead of "degree too large".
    device_build=True builds every trace on the device into one of two device buffers per context
    (no pinned trace buffers, no trace upload); with preflight the check runs on that resident
    trace.  SegmentProof.build_ms is then the wall time of the device build call."""
    idx = list(range(len(plan))) if segments is None else list(segments)
    own = contexts is None
    ctxs = [Context(device) for _ in range(inflight)] if own else list(contexts)
    inflight = len(ctxs)
    if own and preflight:
        for c in ctxs:
            c.set_preflight(True)
    # both buffer slots of every context sized once for the widest, longest segment (the full
    # trace's width bounds every segment layout): the builders then never wait on a context
    # that is proving
    cap = program.width * max(b - a for a, b in plan) * 16
    if device_build:
        bufs = [[c.alloc(cap) for _ in (0, 1)] for c in ctxs]
    else:
        bufs = [[c.trace_buffer(cap, slot) for slot in (0, 1)] for c in ctxs]
    pool = ThreadPoolExecutor(max_workers=max(1, builders))
    out, errors = {}, []
    lock = threading.Lock()

    def build(k, slot, i):
        a, b = plan[i]
        m = b - a
        t0 = time.perf_counter()
        buf = bufs[k][slot]
        if device_build:
            pi, w, sin, sout = ctxs[k].build_segment_device(program, a, b, buf, cap)
        else:
            pi, w, sin, sout = program.segment_into(a, b, buf)
        rec = SegmentProof(i, (a, b), w, pi, sin, sout, proof_options(w, m, queries=queries, blowup=blowup,
                                                                           grind=grind))
        rec.build_ms = (time.perf_counter() - t0) * 1e3
        return rec, buf

    def work(k):
        ctx = ctxs[k]
        mine = idx[k::inflight]
        try:
            nxt = pool.submit(build, k, 0, mine[0]) if mine else None
            for j in range(len(mine)):
                rec, buf = nxt.result()
                nxt = pool.submit(build, k, (j + 1) % 2, mine[j + 1]) if j + 1 < len(mine) else None
                t0 = time.perf_counter()
                prove = ctx.prove_segment_device if device_build else ctx.prove_segment
                rec.proof = prove(buf, rec.width, rec.rows[1] - rec.rows[0], rec.pi, rec.opts)
                rec.prove_ms = (time.perf_counter() - t0) * 1e3
                if on_proof is not None:
                    on_proof(rec)
                with lock:
                    out[rec.index] = rec
        except Exception as e:  # noqa: BLE001  (re-raised below, after every worker stopped)
            with lock:
                errors.append(e)
            if nxt is not None:
                try:
                    nxt.result()
                except Exception:  # noqa: BLE001
                    pass

    th = [threading.Thread(target=work, args=(k,)) for k in range(inflight)]
    try:
        for x in th:
            x.start()
        for x in th:
            x.join()
    finally:
        pool.shutdown(wait=True)
        if device_build:
            for c, pair in zip(ctxs, bufs):
                for d in pair:
                    c.free(d)
        if own:
            for c in ctxs:
                c.close()
    if errors:
        raise errors[0]
    return out


def step_of(r, total: int, main_args=()):
    """The zl1 step proof (ZKLSTP1) of one proved segment (prove.rs:1144-1174)."""
    return step_proof_encode(r.pi, step_info_for(r.pi, r.index, total, r.state_in, r.state_out, main_args=main_args),
                             r.proof)


def steps_of(records, total: int, main_args=()):
    """The zl1 step proofs (ZKLSTP1) of proved segments, in index order (prove.rs:1144-1174)."""
    return [step_of(r, total, main_args) for r in sorted(records, key=lambda r: r.index)]


def prove_chain(program: Program, plan, device: int = 0, inflight: int = 4, builders: int = 8, queries: int = 64,
                blowup: int = 16, grind: int = 16, contexts=None, preflight: bool = False, device_build: bool = False,
                main_args=(), agg_ctx=None, min_security_bits: int = 128, trace_mode: int = AGG_TRACE_VALID,
                agg_queries=None, agg_blowup=None, agg_grind=None, adders: int = 2):
    """`zk-lisp prove` as one operation (prove_chain, recursion.rs:203-213): every segment of
    `plan` proved by prove_program while an aggregation session replays each step proof as soon
    as it exists (on_proof hands the record to one of `adders` threads, which encodes the step and
    adds it at the record's index), then the session's finish.  The session runs on agg_ctx, or on
    a context opened here for it on `device`, so its device work queues beside the segment
    provers' instead of taking their locks.  A child the session refuses does not stop the
    proving; finish raises ZklError for the lowest refused position.  queries /
    blowup / grind are the options of the segment proofs and, unless agg_queries / agg_blowup /
    agg_grind say otherwise, of the aggregation proof (the CLI passes one set to both).
    Returns a dict: artifact, digest, steps (index order), times (AggSession.times()) and
    tail_ms, from the return of the last segment proof to the return of finish."""
    total = len(plan)
    own = agg_ctx is None
    actx = Context(device) if own else agg_ctx
    steps = [None] * total
    last = [0.0]
    lock = threading.Lock()
    # the adds run on threads of their own, so a context goes on to its next segment while the
    # step it just proved is replayed (a 2^16-row child is several ms of host work)
    adders = ThreadPoolExecutor(max_workers=max(1, adders))
    pending = []
    try:
        with AggSession(total, ctx=actx, queries=queries if agg_queries is None else agg_queries,
                        blowup=blowup if agg_blowup is None else agg_blowup,
                        grind=grind if agg_grind is None else agg_grind, min_security_bits=min_security_bits,
                        trace_mode=trace_mode) as session:
            def add(rec):
                step = step_of(rec, total, main_args)
                steps[rec.index] = step
                try:
                    session.add(rec.index, step)
                except ZklError:  # the child's own verdict: finish repeats the lowest refused position
                    pass

            def on_proof(rec):
                t = time.perf_counter()
                with lock:
                    last[0] = max(last[0], t)
                    pending.append(adders.submit(add, rec))

            try:
                prove_program(program, plan, device=device, inflight=inflight, builders=builders, queries=queries,
                              blowup=blowup, grind=grind, contexts=contexts, on_proof=on_proof, preflight=preflight,
                              device_build=device_build)
            finally:  # no add may outlive the session
                wait(pending)
            for f in pending:
                f.result()
            artifact, digest = session.finish()
            tail_ms = (time.perf_counter() - last[0]) * 1e3
            times = session.times()
    finally:
        adders.shutdown(wait=True)
        if own:
            actx.close()
    return {"artifact": artifact, "digest": digest, "steps": steps, "times": times, "tail_ms": tail_ms}
