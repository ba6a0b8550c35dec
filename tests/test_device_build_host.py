"""DESIGN.md §13 -- the device trace builder's staging and its per-cell function, run on the host
(zkl_tracegen_host_fill: the blob the device receives, filled cell by cell through the kernel's
own cell function with the round tables computed by plain loops).  Byte equality with the host
builder Program.segment over the programs and windows of tests/test_segment_builder.py; on a
mismatch the first differing (column, row) is reported."""
import ctypes as C

import pytest

import zkl_hip
from zkl_hip import op
from test_segment_inputs import _program


def mixed_ops():
    """Sponge, RAM and Merkle in one program (width 219): a squeeze after 10 pending absorbs, a
    Merkle path with a MerkleStep between first and last, a store and a load of one address in
    neighbouring levels, Eq on equal and unequal operands, a division by zero."""
    ops = [op("Const", dst=k, imm=11 + 3 * k) for k in range(7)]
    ops += [op("SAbsorbN", regs=[0, 1, 2, 3]), op("SAbsorbN", regs=[4, 5, 6]), op("SAbsorbN", regs=[6, 0, 3]),
            op("SSqueeze", dst=2)]
    ops += [op("Const", dst=7, imm=5), op("Store", addr=7, src=2), op("Load", dst=3, addr=7),
            op("Const", dst=7, imm=2), op("Store", addr=7, src=0), op("Const", dst=7, imm=5), op("Load", dst=4, addr=7),
            op("Eq", dst=5, a=3, b=4), op("Eq", dst=5, a=3, b=0), op("Const", dst=6, imm=0),
            op("DivMod", dst_q=0, dst_r=1, a=3, b=6)]
    ops += [op("Const", dst=4, imm=1), op("Const", dst=5, imm=0), op("Const", dst=6, imm=1),
            op("MerkleStepFirst", leaf_reg=4, dir_reg=5, sib_reg=2), op("MerkleStep", dir_reg=6, sib_reg=3),
            op("MerkleStep", dir_reg=5, sib_reg=1), op("MerkleStepLast", dir_reg=6, sib_reg=0)]
    ops += [op("SAbsorbN", regs=[1]), op("SSqueeze", dst=1), op("Load", dst=2, addr=7), op("End")]
    return ops


def first_diff(got: bytes, want: bytes, rows: int):
    """(column, row) of the first differing cell of two column-major traces, None when equal"""
    if got == want:
        return None
    for i in range(0, len(want), 16):
        if got[i:i + 16] != want[i:i + 16]:
            return divmod(i // 16, rows)
    return (len(want) // 16 // rows, 0)


def host_fill(P, a, b):
    lib = P.lib
    w = C.c_uint32()
    rc = lib.zkl_tracegen_host_fill(C.c_void_p(P.ptr.value), a, b, None, None, C.byref(w), None, None)
    assert rc == 0
    t = (zkl_hip.F128 * (w.value * (b - a)))()
    pi = zkl_hip.AirPublicInputs()
    sin, sout = (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
    rc = lib.zkl_tracegen_host_fill(C.c_void_p(P.ptr.value), a, b, C.cast(t, C.c_void_p), C.byref(pi), C.byref(w),
                                    sin, sout)
    assert rc == 0
    return t, pi, w.value, bytes(sin), bytes(sout)


def check(P, windows):
    for a, b in windows:
        t, pi, w, sin, sout = P.segment(a, b)
        qt, qpi, qw, qin, qout = host_fill(P, a, b)
        assert qw == w
        assert first_diff(bytes(qt), bytes(t), b - a) is None, f"[{a},{b}) first differing (column, row)"
        assert bytes(qpi) == bytes(pi) and (qin, qout) == (sin, sout)


@pytest.mark.parametrize("name,max_rows", [("rollup-bench", 1 << 10), ("rollup-bench", 1 << 12),
                                           ("fib-2pow16-log-n", 1 << 12)])
def test_real_program_segments(name, max_rows):
    P, n_ops = _program(name)
    plan = zkl_hip.plan_segments(n_ops, max_rows)
    # fib-2pow16-log-n: the first segment, the one holding End, one of padding only
    pick = plan if name == "rollup-bench" else [plan[0], plan[32 * (n_ops - 1) // max_rows], plan[-1]]
    check(P, pick)


@pytest.mark.parametrize("name", ["rollup-bench", "fib-2pow16-log-n"])
def test_windows_off_checkpoints(name):
    P, n_ops = _program(name)
    n = P.n_rows
    check(P, [(32 * 33, 32 * 34), (32 * 70, 32 * 72), (32 * 5, 32 * 9), (32 * 100, 32 * 164), (n - 32, n), (0, 32),
              (32 * 31, 32 * 32)])


@pytest.mark.parametrize("prog", ["multiseg", "ram", "alu"])
def test_segment_programs_of_test_segments(prog):
    from test_segments import PID, PROGRAMS
    fn, max_rows = PROGRAMS[prog]
    ops = fn()
    check(zkl_hip.Program(ops, PID), zkl_hip.plan_segments(len(ops), max_rows))


def test_sponge_ram_merkle_program():
    from test_segments import PID
    ops = mixed_ops()
    P = zkl_hip.Program(ops, PID)
    assert P.width == 219 and P.segment_width(0, P.n_rows) == 219
    check(P, [(0, P.n_rows)] + zkl_hip.plan_segments(len(ops), 256))
