"""DESIGN.md §13 -- zkl_segment_inputs: a segment's public inputs, width and VM state hashes
derived from the ops and the pre-pass alone, with no trace.  The reference in every case is the
host builder Program.segment (pinned to the oracle by tests/test_segment_builder.py), which reads
the same values off the trace it wrote.  Same programs and windows as that file.
"""
import ctypes as C
import json
import os

import pytest

import zkl_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = json.load(open(os.path.join(ROOT, "tests", "golden", "programs.json")))


def _prog(name):
    g = G[name]
    ops = [zkl_hip.op(k, **f) for k, f in g["ops"]]
    ma = [(tg, bytes.fromhex(b)) for tg, b in g["cli"]["main_args"]]
    return ops, bytes.fromhex(g["program_id"]), g["cli"]["secret_u64"], ma


_PROGRAMS = {}


def _program(name):
    if name not in _PROGRAMS:
        ops, pid, secret, ma = _prog(name)
        _PROGRAMS[name] = (zkl_hip.Program(ops, pid, secret_args=secret, main_args=ma), len(ops))
    return _PROGRAMS[name]


def _pi_diff(got, want):
    """names of the public-input fields that differ"""
    raw = lambda v: bytes(v) if isinstance(v, (C.Array, C.Structure)) else v  # noqa: E731
    return [f for f, _ in zkl_hip.AirPublicInputs._fields_ if raw(getattr(got, f)) != raw(getattr(want, f))]


def _check(P, windows):
    for a, b in windows:
        _, pi, w, sin, sout = P.segment(a, b)
        qpi, qw, qin, qout = P.segment_inputs(a, b)
        assert qw == w, f"[{a},{b}) width"
        assert bytes(qpi) == bytes(pi), f"[{a},{b}) public inputs differ in {_pi_diff(qpi, pi)}"
        assert (qin, qout) == (sin, sout), f"[{a},{b}) state hashes"


@pytest.mark.parametrize("name", sorted(G))
@pytest.mark.parametrize("max_rows", [1 << 10, 1 << 12, 1 << 16])
def test_every_segment_of_the_real_programs(name, max_rows):
    P, n_ops = _program(name)
    _check(P, zkl_hip.plan_segments(n_ops, max_rows))


@pytest.mark.parametrize("prog", ["multiseg", "ram", "alu"])
def test_segment_programs_of_test_segments(prog):
    from test_segments import PID, PROGRAMS
    fn, max_rows = PROGRAMS[prog]
    ops = fn()
    _check(zkl_hip.Program(ops, PID), zkl_hip.plan_segments(len(ops), max_rows))


@pytest.mark.parametrize("name", sorted(G))
def test_windows_off_checkpoints(name):
    """The window list of test_segment_builder.test_windows_off_checkpoints: starts between the
    32-level checkpoints, one-level windows, padding-only windows, the window holding End."""
    P, n_ops = _program(name)
    n = P.n_rows
    end = 32 * (n_ops - 1)
    _check(P, [(32 * 33, 32 * 34), (32 * 70, 32 * 72), (32 * 5, 32 * 9), (32 * 100, 32 * 164), (n - 32, n),
               (0, 32), (32 * 31, 32 * 32), (end, end + 32)])


def test_rejections():
    ops, pid, secret, ma = _prog("fib-2pow16-log-n")
    P = zkl_hip.Program(ops, pid)
    n = P.n_rows
    for a, b in [(0, 48), (16, 48), (0, 96), (1024, 1024), (0, 2 * n), (n - 32, n + 32)]:
        with pytest.raises(zkl_hip.ZklError):
            P.segment_inputs(a, b)
