"""Trace preflight, device-free half: zkl_eval_transition_row gives the per-constraint values of
one frame in the reference's evaluation order -- the exact resolution step of the device check
 -- pinned against the oracle's orc_api_check_trace (first failing row and
constraint index), plus the C++ mirror's CPU checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "preflight_api_test")


def _rows(zkl_hip, t, w, n, r):
    return zkl_hip.trace_row(t, w, n, r), zkl_hip.trace_row(t, w, n, r + 1)


def _first_nonzero(vals):
    return next((i for i, v in enumerate(vals) if v), None)


def _pair(oracle, seed, log_n, flags=0):
    """The same synthetic segment from the product's generator and the oracle's (equal bytes,
    tests/test_abi.py), each in its own ctypes classes."""
    import zkl_hip
    t, pi, w = zkl_hip.synth_vm_segment(seed, log_n, flags)
    ot, opi, ow = oracle.synth_segment(seed, log_n, flags)
    assert w == ow and bytes(t) == bytes(ot)
    return t, pi, ot, opi, w


def test_register_flip_resolves_to_oracle_constraint(oracle):
    import zkl_hip
    n = 1 << 10
    t, pi, ot, opi, w = _pair(oracle, 0x5EED0001, 10)
    for r in (0, 298, 300):
        assert not any(zkl_hip.eval_transition_row(w, n, pi, r, *_rows(zkl_hip, t, w, n, r))), r
    t[45 * n + 300].lo ^= 1      # register r3 at row 300
    ot[45 * n + 300].lo ^= 1
    rc, row, idx = oracle.check_trace(ot, opi, w, n)
    print("oracle:", rc, row, idx)
    assert (rc, row, idx) == (1, 299, 94)
    vals = zkl_hip.eval_transition_row(w, n, pi, row, *_rows(zkl_hip, t, w, n, row))
    assert len(vals) == oracle.air_info(opi, w, n)[1]
    assert _first_nonzero(vals) == idx
    assert not any(zkl_hip.eval_transition_row(w, n, pi, 298, *_rows(zkl_hip, t, w, n, 298)))


@pytest.mark.parametrize("flags,log_n", [(0, 5), (0, 6), (1, 8), (2, 9), (4, 8), (7, 8)])
def test_constraint_count_matches_oracle_and_valid_rows_vanish(oracle, flags, log_n):
    import zkl_hip
    n = 1 << log_n
    t, pi, ot, opi, w = _pair(oracle, 0x5EED0300 + flags, log_n, flags)
    n_tc = oracle.air_info(opi, w, n)[1]
    for r in sorted({0, 1, 28, 29, min(31, n - 2), n - 2}):   # one row of every selector class, and the last
        vals = zkl_hip.eval_transition_row(w, n, pi, r, *_rows(zkl_hip, t, w, n, r))
        assert len(vals) == n_tc
        assert not any(vals), (r, _first_nonzero(vals))


def test_sponge_flip_reaches_poseidon_block(oracle):
    import zkl_hip
    n = 256
    t, pi, ot, opi, w = _pair(oracle, 0x5EED0055, 8, 1)
    cell = 5 * n + 3 * 32 + 7    # lane 5 of row 3*32+7
    t[cell].lo ^= 1
    ot[cell].lo ^= 1
    rc, row, idx = oracle.check_trace(ot, opi, w, n)
    print("oracle:", rc, row, idx)
    assert rc == 1 and row == 3 * 32 + 6 and idx < 324
    vals = zkl_hip.eval_transition_row(w, n, pi, row, *_rows(zkl_hip, t, w, n, row))
    assert len(vals) == oracle.air_info(opi, w, n)[1]
    assert _first_nonzero(vals) == idx


def test_eval_transition_row_rejects_bad_requests():
    import zkl_hip
    n = 64
    t, pi, w = zkl_hip.synth_vm_segment(0x5EED0001, 6)
    cur, nxt = _rows(zkl_hip, t, w, n, 0)
    with pytest.raises(zkl_hip.ZklError, match="last row") as ei:
        zkl_hip.eval_transition_row(w, n, pi, n - 1, cur, nxt)
    assert ei.value.code == -1
    with pytest.raises(zkl_hip.ZklError, match="width"):
        zkl_hip.eval_transition_row(w - 1, n, pi, 0, cur, nxt)
    with pytest.raises(zkl_hip.ZklError, match="power of two"):
        zkl_hip.eval_transition_row(w, 48, pi, 0, cur, nxt)


def test_report_text_and_json():
    import zkl_hip
    rep = zkl_hip.TraceReport(kind=1, index=94, row=299, pos=299 % 32, value=zkl_hip.F128(1, 0))
    assert str(rep) == "preflight: constraint 94 non-zero at row 299: 1"
    js = rep.to_json()
    assert {"row", "constraint_idx", "constraint_val", "pos", "gates_map", "gates_final", "rounds", "lanes_cur",
            "lanes_next", "lanes_exp", "ram", "vm", "peak_live"} <= set(js)
    assert (js["row"], js["constraint_idx"], js["constraint_val"], len(js["rounds"])) == (299, 94, "1", 27)
    rep = zkl_hip.TraceReport(kind=2, index=3, row=0, column=7, value=zkl_hip.F128(5, 0), expected=zkl_hip.F128(0, 1))
    assert str(rep) == f"preflight: assertion 3 (column 7) fails at row 0: trace 5, expected {1 << 64}"


def _binary():
    if not os.path.exists(BIN):  # host-only g++ build against libzkl_hip.so (zk-lisp_amd/Makefile)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "zk-lisp_amd"), "../tests/cpp/preflight_api_test"],
                       check=True)
    return BIN


def test_cpp_preflight_cpu():
    r = subprocess.run([_binary(), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("ok cpu")
