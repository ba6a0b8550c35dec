"""The host column classifier (zk-lisp_amd/csrc/col_class.h) without a GPU: the stand-alone C++
program on crafted columns, and the library's export of it against a numpy restatement of the
scan's rule on the oracle's synthetic segments.

The device scan (scan_columns_kernel + decode_column_scan) reports the smallest power-of-two period
up to R = min(128, n) of a column whose every row i equals row i mod R, even where that period is
n itself (any 32-row column "has" period 32).  The LDE plan treats a period that is not below n as
general, and the classifier says general for it; so does the restatement here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import zkl_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = zkl_hip.COL_GENERAL
SEED = 0x5EED0001

# (log_n, generator flags) -> width, and the classes {0: zero, P: period P, GEN: general} as counts:
# computed with numpy from the oracle's traces (seed 0x5EED0001); a changed generator shows in the
# restatement's own assertion first
SEGMENTS = {
    (5, 0): (204, {0: 169, GEN: 35}),
    (7, 1): (204, {0: 152, 32: 31, 64: 6, GEN: 15}),
    (8, 0): (204, {0: 145, 32: 31, 128: 7, GEN: 21}),
    (10, 3): (212, {0: 92, 32: 29, GEN: 91}),
    (8, 7): (219, {0: 148, 32: 29, GEN: 42}),
}


def numpy_classes(mat):
    """mat: (W, n, 2) uint64.  The scan's rule, restated: structured iff every row i equals row
    i mod R; then zero, or the smallest power of two P with row t = row t - P over the first R rows
    (R itself when none is smaller); a period that is not below n is general."""
    w, n, _ = mat.shape
    r = min(128, n)
    out = []
    for c in range(w):
        col = mat[c]
        if not np.array_equal(col, np.tile(col[:r], (n // r, 1))):
            out.append(GEN)
            continue
        head = col[:r]
        if not head.any():
            out.append(0)
            continue
        p = 1
        while p < r and not np.array_equal(head[p:], head[:-p]):
            p *= 2
        out.append(p if p < n else GEN)
    return out


def test_classifier_host_program(tmp_path):
    """tests/cpp/col_class_test.cpp: crafted columns at n = 32 .. 4096 (zero, NULL, single rows,
    constants, exact periods, a period equal to n, a late mismatch, hi-only differences) and the
    bit-word restatement of the device scan; built with the address and undefined-behaviour
    sanitizers where the host compiler has them (host code only)."""
    src = os.path.join(ROOT, "tests", "cpp", "col_class_test.cpp")
    exe = str(tmp_path / "col_class_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", src, "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                      capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("col_class_test ok")


@pytest.mark.parametrize("log_n,flags", sorted(SEGMENTS))
def test_classes_of_oracle_segments(oracle, log_n, flags):
    n = 1 << log_n
    width, want = SEGMENTS[log_n, flags]
    trace, _, w = oracle.synth_segment(SEED, log_n, flags)
    assert w == width
    mat = np.frombuffer(trace, dtype=np.uint64).reshape(w, n, 2)
    ref = numpy_classes(mat)
    counts = {k: ref.count(k) for k in set(ref)}
    assert counts == want
    # separately allocated columns, every second zero column passed as None
    cols, zeros = [], 0
    for c in range(w):
        if ref[c] == 0:
            zeros += 1
            if zeros % 2:
                cols.append(None)
                continue
        cols.append((C.c_uint8 * (n * 16)).from_buffer_copy(mat[c].tobytes()))
    assert zkl_hip.classify_columns(cols, n) == ref


def test_classify_rejects_bad_shapes():
    col = (C.c_uint8 * (48 * 16))()
    with pytest.raises(zkl_hip.ZklError):
        zkl_hip.classify_columns([col], 48)
    with pytest.raises(zkl_hip.ZklError):
        zkl_hip.classify_columns([], 32)
