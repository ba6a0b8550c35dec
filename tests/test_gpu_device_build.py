"""DESIGN.md §13 -- segment traces built on the device (zkl_hip_build_segment_trace_device).

The reference in every comparison is the host builder Program.segment (pinned to the oracle by
tests/test_segment_builder.py); the tolerance is byte equality of the whole trace, the public
inputs, the width and the two state hashes.  Before every build the destination is filled with
0xFF bytes, so a cell the kernel does not write shows.  On a mismatch the first differing
(column, row) is reported.
"""
import ctypes as C
import threading

import pytest

import zkl_hip
from zkl_hip.program import prove_program, steps_of
from test_device_build_host import first_diff, mixed_ops
from test_segment_inputs import _program
from test_segments import PID, PROGRAMS

pytestmark = pytest.mark.gpu


class Dev:
    """One 0xFF-filled device buffer, reused by every build of a test."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = ctx.alloc(nbytes)
        self.ff = (C.c_uint8 * nbytes)()
        C.memset(self.ff, 0xFF, nbytes)

    def build(self, P, a, b):
        self.ctx.upload(self.ptr, self.ff, self.nbytes)
        pi, w, sin, sout = self.ctx.build_segment_device(P, a, b, self.ptr, self.nbytes)
        return self.ctx.download(self.ptr, w * (b - a) * 16), pi, w, sin, sout

    def close(self):
        self.ctx.free(self.ptr)


def check(ctx, P, windows):
    dev = Dev(ctx, max(P.segment_width(a, b) * (b - a) * 16 for a, b in windows))
    try:
        for a, b in windows:
            t, pi, w, sin, sout = P.segment(a, b)
            got, qpi, qw, qin, qout = dev.build(P, a, b)
            assert qw == w, f"[{a},{b}) width"
            assert first_diff(got, bytes(t), b - a) is None, f"[{a},{b}) first differing (column, row)"
            assert bytes(qpi) == bytes(pi), f"[{a},{b}) public inputs"
            assert (qin, qout) == (sin, sout), f"[{a},{b}) state hashes"
    finally:
        dev.close()


# ---- 1. small programs ----------------------------------------------------------------------------
@pytest.mark.parametrize("prog", ["alu", "ram", "multiseg"])
def test_small_programs(gpu_ctx, prog):
    fn, max_rows = PROGRAMS[prog]
    ops = fn()
    P = zkl_hip.Program(ops, PID)
    plan = zkl_hip.plan_segments(len(ops), max_rows)
    if prog == "multiseg":
        assert sorted(P.segment_width(a, b) for a, b in plan) == [204, 211]
    check(gpu_ctx, P, plan)


def test_sponge_ram_merkle_program(gpu_ctx):
    ops = mixed_ops()
    P = zkl_hip.Program(ops, PID)
    assert P.width == 219 and P.segment_width(0, P.n_rows) == 219
    check(gpu_ctx, P, [(0, P.n_rows)] + zkl_hip.plan_segments(len(ops), 256))


# ---- 2. real programs -----------------------------------------------------------------------------
def test_rollup_bench_1024_row_plan(gpu_ctx):
    P, n_ops = _program("rollup-bench")
    plan = zkl_hip.plan_segments(n_ops, 1 << 10)
    assert len(plan) == 64 and {P.segment_width(a, b) for a, b in plan} == {204, 212}
    check(gpu_ctx, P, plan)


def test_fib_4096_row_segments(gpu_ctx):
    P, n_ops = _program("fib-2pow16-log-n")
    plan = zkl_hip.plan_segments(n_ops, 1 << 12)
    check(gpu_ctx, P, [plan[0], plan[32 * (n_ops - 1) // 4096], plan[-1]])  # first, End's, padding only


@pytest.mark.parametrize("name", ["rollup-bench", "fib-2pow16-log-n"])
def test_windows_off_checkpoints(gpu_ctx, name):
    P, _ = _program(name)
    n = P.n_rows
    check(gpu_ctx, P, [(32 * 33, 32 * 34), (32 * 70, 32 * 72), (32 * 5, 32 * 9), (32 * 100, 32 * 164), (n - 32, n),
                       (0, 32), (32 * 31, 32 * 32)])


# ---- 3. one full-size grid ------------------------------------------------------------------------
def test_full_size_segment(gpu_ctx):
    P, n_ops = _program("rollup-bench")
    a, b = zkl_hip.plan_segments(n_ops, 1 << 16)[0]
    assert b - a == 1 << 16  # 2048 levels
    check(gpu_ctx, P, [(a, b)])


# ---- 4. proof parity ------------------------------------------------------------------------------
def _proof_cases():
    fn, max_rows = PROGRAMS["multiseg"]
    ops = fn()
    P = zkl_hip.Program(ops, PID)
    cases = [(P, a, b) for a, b in zkl_hip.plan_segments(len(ops), max_rows)]
    R, n_ops = _program("rollup-bench")
    a, b = zkl_hip.plan_segments(n_ops, 1 << 10)[0]
    assert R.segment_width(a, b) == 212
    return cases + [(R, a, b)]


def test_proofs_equal_host_built(gpu_ctx):
    for P, a, b in _proof_cases():
        t, pi, w, _, _ = P.segment(a, b)
        opts = zkl_hip.proof_options(w, b - a, queries=8, grind=4)
        want = gpu_ctx.prove_segment(t, w, b - a, pi, opts)
        dev = Dev(gpu_ctx, w * (b - a) * 16)
        try:
            gpu_ctx.upload(dev.ptr, dev.ff, dev.nbytes)
            qpi, qw, _, _ = gpu_ctx.build_segment_device(P, a, b, dev.ptr, dev.nbytes)
            assert gpu_ctx.prove_segment_device(dev.ptr, qw, b - a, qpi, opts) == want, f"[{a},{b}) proof"
            gpu_ctx.set_preflight(True)
            try:
                assert gpu_ctx.prove_segment_device(dev.ptr, qw, b - a, qpi, opts) == want, f"[{a},{b}) preflight"
            finally:
                gpu_ctx.set_preflight(False)
        finally:
            dev.close()


# ---- 5. the segment loop --------------------------------------------------------------------------
def test_prove_program_device_build():
    P, n_ops = _program("rollup-bench")
    plan = zkl_hip.plan_segments(n_ops, 1 << 10)
    seg = [0, 1, 40, 63]  # 212- and 204-wide
    kw = dict(inflight=2, builders=2, segments=seg, queries=8, grind=4)
    host = prove_program(P, plan, **kw)
    dev = prove_program(P, plan, device_build=True, preflight=True, **kw)
    assert sorted(dev) == sorted(host) == seg
    for i in seg:
        assert dev[i].proof == host[i].proof, i
        assert (dev[i].width, dev[i].state_in, dev[i].state_out) == (host[i].width, host[i].state_in, host[i].state_out)
        assert bytes(dev[i].pi) == bytes(host[i].pi)
        assert dev[i].build_ms > 0
    assert steps_of(dev.values(), len(plan)) == steps_of(host.values(), len(plan))


# ---- 6. concurrency -------------------------------------------------------------------------------
def test_two_contexts_one_program(gpu_ctx):
    P, n_ops = _program("rollup-bench")
    plan = zkl_hip.plan_segments(n_ops, 1 << 10)
    mine = {0: plan[0:8], 1: plan[8:16]}
    other = zkl_hip.Context(0)
    got, errors = {}, []

    def work(k, ctx):
        try:
            dev = Dev(ctx, 212 * 1024 * 16)
            try:
                got[k] = [dev.build(P, a, b) for a, b in mine[k]]
            finally:
                dev.close()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=work, args=(0, gpu_ctx)), threading.Thread(target=work, args=(1, other))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    other.close()
    assert not errors, errors
    for k in (0, 1):
        for (a, b), (trace, pi, w, sin, sout) in zip(mine[k], got[k]):
            t, hpi, hw, hin, hout = P.segment(a, b)
            assert w == hw and first_diff(trace, bytes(t), b - a) is None, f"[{a},{b})"
            assert bytes(pi) == bytes(hpi) and (sin, sout) == (hin, hout)


# ---- 7. rejections --------------------------------------------------------------------------------
def test_rejections(gpu_ctx):
    P, n_ops = _program("fib-2pow16-log-n")
    n = P.n_rows
    need = 204 * 1024 * 16
    dev = Dev(gpu_ctx, need)
    try:
        gpu_ctx.upload(dev.ptr, dev.ff, need)
        for a, b in [(0, 48), (16, 48), (0, 96), (1024, 1024), (0, 2 * n), (n - 32, n + 32)]:
            with pytest.raises(zkl_hip.ZklError):
                gpu_ctx.build_segment_device(P, a, b, dev.ptr, need)
        with pytest.raises(zkl_hip.ZklError):
            gpu_ctx.build_segment_device(P, 0, 1024, dev.ptr, need - 1)
        assert gpu_ctx.download(dev.ptr, need) == bytes(dev.ff)
        assert gpu_ctx.build_segment_device(P, 0, 1024, None) == (None, 204, None, None)
        assert gpu_ctx.build_segment_device(P, 0, 1024, dev.ptr, need)[1] == 204
    finally:
        dev.close()
