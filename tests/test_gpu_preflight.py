"""Trace preflight on the GPU (zkl_hip_check_trace*): the device filter
plus the host resolution report exactly what the CPU oracle's orc_api_check_trace reports -- the
first failing row and the first non-zero constraint of that row, or the first failing assertion
when every transition holds -- on all four segment layouts, and the opt-in step in front of the
prove calls refuses a bad trace by name without changing the bytes of a good one's proof.
Expected values come from the oracle at run time."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "preflight_api_test")


class Case:
    """One synthetic segment from the product's generator and the oracle's (equal bytes), each in
    its own ctypes classes; every mutation is applied to both."""

    def __init__(self, oracle, seed, log_n, flags=0):
        import zkl_hip
        self.oracle, self.n = oracle, 1 << log_n
        self.t, self.pi, self.w = zkl_hip.synth_vm_segment(seed, log_n, flags)
        self.ot, self.opi, ow = oracle.synth_segment(seed, log_n, flags)
        assert ow == self.w and bytes(self.t) == bytes(self.ot) and bytes(self.pi) == bytes(self.opi)

    def flip(self, col, row, bit=1):
        self.t[col * self.n + row].lo ^= bit
        self.ot[col * self.n + row].lo ^= bit

    def want(self):
        return self.oracle.check_trace(self.ot, self.opi, self.w, self.n)

    def check(self, ctx, seed=0):
        return ctx.check_trace(self.t, self.w, self.n, self.pi, seed)

    def assert_agrees(self, ctx, seed=0):
        """The device report against the oracle's (rc, row, idx); returns both."""
        import zkl_hip
        rc, row, idx = self.want()
        rep = self.check(ctx, seed)
        print("oracle:", (rc, row, idx), "device:", rep)
        if rc == 0:
            assert rep is None
        elif idx >= 0:
            assert (rep.kind, rep.row, rep.index, rep.pos) == (1, row, idx, row % 32)
            vals = zkl_hip.eval_transition_row(self.w, self.n, self.pi, row, zkl_hip.trace_row(self.t, self.w, self.n, row),
                                               zkl_hip.trace_row(self.t, self.w, self.n, row + 1))
            assert rep.value_int == vals[idx] != 0 and not any(vals[:idx])
            assert str(rep) == f"preflight: constraint {idx} non-zero at row {row}: {vals[idx]}"
        else:
            assert (rep.kind, rep.row, rep.index) == (2, row, -1 - idx)
            cell = self.t[rep.column * self.n + row]
            assert rep.value_int == cell.lo | (cell.hi << 64) != rep.expected_int
        return rep, (rc, row, idx)


@pytest.mark.parametrize("flags,log_n", [(0, 5), (0, 6), (1, 8), (2, 9), (4, 8), (7, 8)])
def test_valid_traces_pass(gpu_ctx, oracle, flags, log_n):
    """All four layouts; n = 32 is a single partial workgroup with 31 live rows.  A valid trace
    does not satisfy the wrap-around transition, so this also shows row n - 1 is exempt."""
    c = Case(oracle, 0x5EED0300 + flags, log_n, flags)
    assert c.want() == (0, 0, 0)
    assert c.check(gpu_ctx) is None
    assert c.check(gpu_ctx, seed=0xC0FFEE12345) is None
    assert gpu_ctx.last_trace_report() is None


def test_first_failure_not_any_failure(gpu_ctx, oracle):
    n = 1 << 10
    c = Case(oracle, 0x5EED0001, 10)
    c.flip(45, 700)
    c.flip(45, 300)
    rep, want = c.assert_agrees(gpu_ctx)
    assert want == (1, 299, 94)
    assert c.check(gpu_ctx, seed=99).row == 299
    c.flip(45, 300)                       # only row 700 left
    rep, want = c.assert_agrees(gpu_ctx)
    assert want == (1, 700, 102)
    c.flip(45, 700)
    c.flip(45, n - 1)                     # the last checked row: its nxt is the exempt row
    rep, want = c.assert_agrees(gpu_ctx)
    assert want == (1, n - 2, 94)


def test_assertions(gpu_ctx, oracle):
    n = 64
    c = Case(oracle, 0x5EED0001, 6)
    c.pi.pc_init.lo += 1
    c.opi.pc_init.lo += 1
    rep, (rc, row, idx) = c.assert_agrees(gpu_ctx)
    assert (rc, row) == (1, 0) and idx < 0
    assert rep.expected_int == c.pi.pc_init.lo | (c.pi.pc_init.hi << 64)
    assert str(rep).startswith(f"preflight: assertion {rep.index} (column {rep.column}) fails at row 0: trace ")
    # an assertion on the exempt last row
    c = Case(oracle, 0x5EED0001, 6)
    c.pi.rom_s_out[0].lo ^= 1
    c.opi.rom_s_out[0].lo ^= 1
    rep, (rc, row, idx) = c.assert_agrees(gpu_ctx)
    assert (rep.kind, rep.row) == (2, n - 1)
    # a failing transition takes precedence over a failing assertion, as in the oracle
    c = Case(oracle, 0x5EED0001, 6)
    c.pi.pc_init.lo += 1
    c.opi.pc_init.lo += 1
    c.flip(42 + 3, 40)
    rep, (rc, row, idx) = c.assert_agrees(gpu_ctx)
    assert rep.kind == 1 and idx >= 0


def test_poseidon_block(gpu_ctx, oracle):
    """The two-kernel path of the Poseidon layouts, and the expected-lanes snapshot."""
    c = Case(oracle, 0x5EED0055, 8, 1)
    c.flip(5, 3 * 32 + 7)
    rep, (rc, row, idx) = c.assert_agrees(gpu_ctx)
    assert rc == 1 and idx < 324
    js = rep.to_json()
    assert rep.lanes_exp_valid and js["lanes_exp"] is not None and js["ram"] is None
    # lane 5 is neither l, r, c0 nor c1: those four still follow the round function
    assert js["lanes_exp"] == js["lanes_next"]


def test_ram_block(gpu_ctx, oracle):
    """test_ram_corruption_detected's input: a read that differs from the last write."""
    n = 1 << 9
    c = Case(oracle, 0x5EED0301, 9, 2)
    s_on, s_val, s_w = 149, 152, 153
    row = next(r for r in range(n) if c.t[s_on * n + r].lo == 1 and c.t[s_w * n + r].lo == 0
               and (c.t[s_val * n + r].lo | c.t[s_val * n + r].hi))
    c.flip(s_val, row)
    rep, (rc, _, idx) = c.assert_agrees(gpu_ctx)
    assert rc == 1 and rep.kind == 1
    js = rep.to_json()
    assert rep.ram_valid and set(js["ram"]) == {"sorted", "addr_cur", "addr_next", "clk_cur", "clk_next", "val", "is_write",
                                                "last_cur", "last_next", "gp_unsorted_cur", "gp_unsorted_next",
                                                "gp_sorted_cur", "gp_sorted_next"}


def test_merkle_block(gpu_ctx, oracle):
    """test_merkle_root_binding's input: the public root differs from the path's."""
    c = Case(oracle, 0x99, 8, 4)
    c.pi.merkle_root[0] ^= 1
    c.opi.merkle_root[0] ^= 1
    rep, (rc, row, idx) = c.assert_agrees(gpu_ctx)
    assert (rc, row) == (1, 5 * 32 + 28) and rep.kind == 1


def test_entry_points_agree(gpu_ctx, oracle):
    c = Case(oracle, 0x5EED0001, 10)
    nbytes = c.w * c.n * 16
    d = gpu_ctx.alloc(nbytes)
    try:
        for corrupt in (False, True):
            if corrupt:
                c.flip(45, 300)
            gpu_ctx.upload(d, c.t, nbytes)
            host, dev = c.check(gpu_ctx), gpu_ctx.check_trace_device(d, c.w, c.n, c.pi)
            assert (host is None) == (dev is None) == (not corrupt)
            if corrupt:
                assert bytes(host) == bytes(dev) and (dev.row, dev.index) == (299, 94)
    finally:
        gpu_ctx.free(d)


def test_request_errors(gpu_ctx, oracle):
    import zkl_hip
    c = Case(oracle, 0x5EED0001, 6)
    with pytest.raises(zkl_hip.ZklError, match="width") as ei:
        gpu_ctx.check_trace(c.t, c.w - 1, c.n, c.pi)
    assert ei.value.code == -1
    with pytest.raises(zkl_hip.ZklError, match="power of two"):
        gpu_ctx.check_trace(c.t, c.w, 48, c.pi)


def test_prove_integration(oracle):
    """n = 2^8, 32 queries, grind 8: proof bytes with the preflight on equal those with it off,
    from both entry points; a corrupted 2^10 trace is refused by name with it on, and with the
    prover's own message with it off."""
    import zkl_hip
    ctx = zkl_hip.Context(0)
    try:
        assert not ctx.preflight
        n = 1 << 8
        t, pi, w = zkl_hip.synth_vm_segment(0x5EED0001, 8)
        opts = zkl_hip.proof_options(w, n, queries=32, grind=8)
        d = ctx.alloc(w * n * 16)
        ctx.upload(d, t, w * n * 16)
        off_host, off_dev = ctx.prove_segment(t, w, n, pi, opts), ctx.prove_segment_device(d, w, n, pi, opts)
        assert off_host == off_dev
        ctx.set_preflight(True)
        assert ctx.preflight
        assert ctx.prove_segment(t, w, n, pi, opts) == off_host
        assert ctx.prove_segment_device(d, w, n, pi, opts) == off_host
        buf = bytearray(len(off_host))
        assert ctx.prove_segment_device_into(d, w, n, pi, opts, buf) == len(off_host) and bytes(buf) == off_host
        assert ctx.last_trace_report() is None
        ctx.free(d)

        n = 1 << 10
        t, pi, w = zkl_hip.synth_vm_segment(0x5EED0001, 10)
        t[45 * n + 300].lo ^= 1
        opts = zkl_hip.proof_options(w, n, queries=32, grind=8)
        d = ctx.alloc(w * n * 16)
        ctx.upload(d, t, w * n * 16)
        for prove in (lambda: ctx.prove_segment(t, w, n, pi, opts), lambda: ctx.prove_segment_device(d, w, n, pi, opts)):
            with pytest.raises(zkl_hip.ZklError, match="preflight: constraint 94 non-zero at row 299: ") as ei:
                prove()
            assert ei.value.code == -1
            rep = ctx.last_trace_report()
            assert (rep.kind, rep.row, rep.index) == (1, 299, 94) and str(rep) in str(ei.value)
        ctx.set_preflight(False)
        for prove in (lambda: ctx.prove_segment(t, w, n, pi, opts), lambda: ctx.prove_segment_device(d, w, n, pi, opts)):
            with pytest.raises(zkl_hip.ZklError, match="degree too large"):
                prove()
        ctx.free(d)
    finally:
        ctx.close()


def test_cpp_preflight_gpu():
    if not os.path.exists(BIN):  # host-only g++ build against libzkl_hip.so (zk-lisp_amd/Makefile)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "zk-lisp_amd"), "../tests/cpp/preflight_api_test"],
                       check=True)
    r = subprocess.run([BIN, "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("ok gpu preflight: preflight: constraint 94 non-zero at row 299: ")
