"""Column structure in the trace LDE, DEEP and OOD: the general columns through one
launch group and a column map, the periodic columns as a small LDE tiled over the column, the
bookkeeping of what a context left zero, and whole proofs against the oracle's.

The periodic identity is checked in Python integers by naive evaluation; the LDE stage against
the same call with the switch off and against a Python transform over the oracle's roots of
unity; the proofs against the oracle's proofs, computed once per module."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import zkl_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = zkl_hip.COL_GENERAL
P_FIELD = 2**128 - 45 * 2**40 + 1
SHIFT = 3  # the LDE coset is 3 * <w_N>


def _bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def _lde_pos(r, n_rows):
    """kernels.h lde_pos: position of natural row r in the split layout."""
    log_s = n_rows.bit_length() - 1 - 8
    s = 1 << log_s
    big_l, t = r & (s - 1), r >> log_s
    lo = big_l & 7
    return (big_l - lo) + (lo >> 1) + ((t & 1) << 2) + (((t >> 1) + ((lo & 1) << 7)) << log_s)


def _fe_buf(vals):
    return (C.c_uint8 * (16 * len(vals))).from_buffer_copy(b"".join(v.to_bytes(16, "little") for v in vals))


def _ints(raw):
    a = np.frombuffer(raw, dtype=np.uint64).reshape(-1, 2)
    return [int(lo) | (int(hi) << 64) for lo, hi in a]


@pytest.fixture
def pm_policy(gpu_ctx):
    """Every Poseidon level of >= 32 states on the matrix-core permutation (the prefix skip lives in
    its row kernel); the default policy afterwards."""
    lib = zkl_hip.load_library()
    assert lib.zkl_hip_set_hash_policy(1, 32) == 0
    yield
    assert lib.zkl_hip_set_hash_policy(1, 1 << 14) == 0


# ------------------------------------------------------------------ CPU: the periodic identity
def _interpolate_naive(vals, w):
    """Coefficients of the polynomial with f(w^i) = vals[i], w a primitive len(vals)-th root."""
    m, p = len(vals), P_FIELD
    wi, mi = pow(w, p - 2, p), pow(m, p - 2, p)
    return [sum(v * pow(wi, i * k, p) for i, v in enumerate(vals)) * mi % p for k in range(m)]


def _eval(coefs, x):
    acc = 0
    for c in reversed(coefs):
        acc = (acc * x + c) % P_FIELD
    return acc


@pytest.mark.parametrize("period", [1, 2, 8, 32])
def test_periodic_identity(oracle, period):
    """n = 64, blowup 4.  A column v[i] = v[i mod P] has f(x) = h(x^(n/P)): LDE row r is row r mod
    B P of the B P-point coset evaluation of h with shift 3^(n/P), and in the bit-reversed, coset-
    scaled coef layout (coef[bitrev_n(k)] = c_k 3^k) the non-zero entries are the first P, entry
    bitrev_P(j) = h_j 3^(j n/P): what periodic_lde_kernel computes and where it writes."""
    p, n, blow = P_FIELD, 64, 4
    big_n, log_n = n * blow, 6
    w_big = oracle.root_of_unity(8)
    assert pow(w_big, big_n, p) == 1 and pow(w_big, big_n // 2, p) != 1
    g = pow(w_big, blow, p)
    rng = random.Random(period)
    base = [rng.randrange(1, p) for _ in range(period)]
    f = _interpolate_naive([base[i % period] for i in range(n)], g)
    dense_lde = [_eval(f, SHIFT * pow(w_big, r, p) % p) for r in range(big_n)]
    dense_coef = [0] * n
    for k in range(n):
        dense_coef[_bitrev(k, log_n)] = f[k] * pow(SHIFT, k, p) % p
    # the small transform, as the kernel states it
    log_p, bp = period.bit_length() - 1, blow * period
    h = _interpolate_naive(base, pow(g, n // period, p))
    c = [h[j] * pow(SHIFT, j * (n // period), p) % p for j in range(period)]
    w_bp = pow(w_big, big_n // bp, p)
    small = [sum(c[j] * pow(w_bp, r * j, p) for j in range(period)) % p for r in range(bp)]
    assert [small[r % bp] for r in range(big_n)] == dense_lde
    sparse = [0] * n
    for j in range(period):
        sparse[_bitrev(j, log_p)] = c[j]
    assert sparse == dense_coef  # so every dense entry from P on is zero


def test_plan_and_bookkeeping_host_program(tmp_path):
    """tests/cpp/lde_plan_test.cpp: the routine's plan (column map, period groups, clears) and the
    book of what the context left zero, on crafted class vectors; built with the address and
    undefined-behaviour sanitizers where the host compiler has them (host code only)."""
    src = os.path.join(ROOT, "tests", "cpp", "lde_plan_test.cpp")
    exe = str(tmp_path / "lde_plan_test")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", src, "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                      capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "lde_plan_test ok"


# ------------------------------------------------------------------ the reference transform
def _ntt(a, w):
    """In-order radix-2 transform: out[k] = sum_j a[j] w^(jk)."""
    p, m = P_FIELD, len(a)
    bits = m.bit_length() - 1
    a = [a[_bitrev(i, bits)] for i in range(m)]
    size = 2
    while size <= m:
        wl = pow(w, m // size, p)
        tw = [1] * (size // 2)
        for i in range(1, size // 2):
            tw[i] = tw[i - 1] * wl % p
        for s in range(0, m, size):
            for i in range(size // 2):
                u, v = a[s + i], a[s + i + size // 2] * tw[i] % p
                a[s + i], a[s + i + size // 2] = (u + v) % p, (u - v) % p
        size *= 2
    return a


def _reference_lde(oracle, col, n, blow):
    """(coef column in the device layout, LDE column in natural order) of one trace column."""
    p, big_n = P_FIELD, n * blow
    log_n = n.bit_length() - 1
    w_big = oracle.root_of_unity(big_n.bit_length() - 1)
    g = pow(w_big, blow, p)
    inv_n = pow(n, p - 2, p)
    f = [x * inv_n % p for x in _ntt(col, pow(g, p - 2, p))]
    scaled, s = [], 1
    for k in range(n):
        scaled.append(f[k] * s % p)
        s = s * SHIFT % p
    coef = [0] * n
    for k in range(n):
        coef[_bitrev(k, log_n)] = scaled[k]
    return coef, _ntt(scaled + [0] * (big_n - n), w_big)


def _column(rng, n, k):
    p = P_FIELD
    if k == GEN:
        return [rng.randrange(p) for _ in range(n)]
    if k == 0:
        return [0] * n
    base = [rng.randrange(1, p) for _ in range(k)]
    if k > 1:
        base[k // 2] = (base[0] + 1) % p  # the smallest period is k itself
    return [base[i % k] for i in range(n)]


# short runs of every class, first and last column of several; 24 columns
STAGE_SPEC = [0, GEN, 1, 0, 2, GEN, 32, 0, 128, GEN, 0, 0, 2, 1, GEN, 128, 0, 32, GEN, GEN, 0, 8, 128, 1]
STAGE_SHAPES = {
    # N = 2^11: the smallest shape whose last pass stores the split layout
    "n256_b8_split": (256, 8, True, 1),
    "n1024_b16_natural": (1024, 16, False, 0),
    # period 128 equals n: those columns take the general path (every 128-row column "has" it)
    "n128_b16_period_is_n": (128, 16, False, 0),
}


def _run_stage(ctx, d_v, ncols, n, blow, d_c, d_l, want_split):
    sp = ctx.lde_columns(d_v, ncols, n, blow, d_c, d_l, want_split=want_split)
    return sp, ctx.download(d_c, ncols * n * 16), ctx.download(d_l, ncols * n * blow * 16)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(STAGE_SHAPES))
def test_lde_stage_matches_dense_and_reference(oracle, gpu_ctx, shape):
    n, blow, want_split, layout = STAGE_SHAPES[shape]
    rng = random.Random(n * blow)
    ncols, big_n = len(STAGE_SPEC), n * blow
    cols = [_column(rng, n, k) for k in STAGE_SPEC]
    raw = _fe_buf([v for c in cols for v in c])
    d_v, d_c, d_l = gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(len(raw) * blow)
    try:
        gpu_ctx.upload(d_v, raw, len(raw))
        want_per = [k if (k in (0, GEN) or k < n) else GEN for k in STAGE_SPEC]
        got_per = gpu_ctx.scan_columns(d_v, ncols, n)
        if n > 128:
            assert got_per == want_per
        else:  # every column of 128 rows has "period" 128 at most: none below n but the crafted
            assert [x if x < n else GEN for x in got_per] == want_per
        sp, coef, lde = _run_stage(gpu_ctx, d_v, ncols, n, blow, d_c, d_l, want_split)
        assert sp == layout
        with zkl_hip.column_structure(False):
            sp0, coef0, lde0 = _run_stage(gpu_ctx, d_v, ncols, n, blow, d_c, d_l, want_split)
        assert sp0 == layout
        assert coef == coef0
        assert lde == lde0
    finally:
        for d in (d_v, d_c, d_l):
            gpu_ctx.free(d)
    got_c, got_l = _ints(coef), _ints(lde)
    pos = [_lde_pos(r, big_n) if layout else r for r in range(big_n)]
    for c, col in enumerate(cols):
        ref_c, ref_l = _reference_lde(oracle, col, n, blow)
        assert got_c[c * n:(c + 1) * n] == ref_c, c
        assert [got_l[c * big_n + q] for q in pos] == ref_l, c


@pytest.mark.gpu
def test_lde_stage_buffer_reuse_across_class_changes(gpu_ctx):
    """One context, the same d_coeffs / d_lde, six matrices in which every column walks general ->
    period 32 -> zero -> period 2 -> general -> zero (each column starting at another step, so
    every call mixes the classes): the bytes equal the dense result after every call.  A stale
    coef tail behind a periodic head, or a slice wrongly remembered as zero, shows here.  All
    matrices are resident before the first call and the dense results are taken first, so nothing
    but the calls under test touches the context's book in between."""
    n, blow, ncols, steps = 256, 8, 8, 6
    walk = [GEN, 32, 0, 2, GEN, 0]
    rng = random.Random(0xB00C)
    size = ncols * n * 16
    mats = []
    for s in range(steps):
        mats.append(_fe_buf([v for c in range(ncols) for v in _column(rng, n, walk[(s + c) % steps])]))
    d_vs = [gpu_ctx.alloc(size) for _ in range(steps)]
    d_c, d_l = gpu_ctx.alloc(size), gpu_ctx.alloc(size * blow)
    try:
        for d, m in zip(d_vs, mats):
            gpu_ctx.upload(d, m, size)
        dense = []
        with zkl_hip.column_structure(False):
            for d in d_vs:
                dense.append(_run_stage(gpu_ctx, d, ncols, n, blow, d_c, d_l, True))
        for s, d in enumerate(d_vs):
            assert gpu_ctx.scan_columns(d, ncols, n) == [walk[(s + c) % steps] for c in range(ncols)]
            got = _run_stage(gpu_ctx, d, ncols, n, blow, d_c, d_l, True)
            assert got[0] == dense[s][0] == 1, s
            assert got[1] == dense[s][1], s
            assert got[2] == dense[s][2], s
        # and once more round the walk without a dense call before it
        for s, d in enumerate(d_vs):
            got = _run_stage(gpu_ctx, d, ncols, n, blow, d_c, d_l, True)
            assert got[1:] == dense[s][1:], s
    finally:
        for d in d_vs + [d_c, d_l]:
            gpu_ctx.free(d)


# ------------------------------------------------------------------ GPU: whole proofs
QUERIES, GRIND = 32, 4
SEEDS = {"structured": (0x5EED0001, 0), "unstructured": (0x5EED0001, 1)}
# (log_n, blowup) -> the layout its trace LDE runs in (asserted below through the stage call at
# the same n and blowup): N = 2^11 stores the split layout, N = 2^14 natural order (its DIT stages
# split 8 + 2, and only a last pass of 8 stages knows the layout)
PROOF_SHAPES = {(8, 8): 1, (10, 16): 0}


def _options(w, log_n, blow, np_):
    o = zkl_hip.proof_options(w, 1 << log_n, queries=QUERIES, blowup=blow, grind=GRIND)
    o.num_partitions, o.hash_rate = np_, 16
    return o


@pytest.fixture(scope="module")
def reference_proofs(oracle):
    """The oracle's proofs of both segments at both shapes, 4 and 1 partitions, computed once."""
    out = {}
    oracle.set_threads(16)
    try:
        for (log_n, blow) in PROOF_SHAPES:
            for kind, (seed, flags) in SEEDS.items():
                ot, opi, w = oracle.synth_segment(seed, log_n, flags)
                for np_ in (4, 1):
                    o = _options(w, log_n, blow, np_)
                    oo = oracle.ProofOptions(*[getattr(o, f) for f, _ in o._fields_])
                    out[log_n, blow, kind, np_] = oracle.prove(ot, w, 1 << log_n, opi, oo)
    finally:
        oracle.set_threads(1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(PROOF_SHAPES))
def test_proof_shape_layout(gpu_ctx, shape):
    """The layout each proof shape's trace LDE runs in, from the stage call at the same n and
    blowup (the prover asks for the split layout whenever the last pass can store it)."""
    log_n, blow = shape
    n, ncols = 1 << log_n, 4
    rng = random.Random(log_n)
    raw = _fe_buf([v for k in (GEN, 0, 32, GEN) for v in _column(rng, n, k)])
    d_v, d_c, d_l = gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(len(raw) * blow)
    try:
        gpu_ctx.upload(d_v, raw, len(raw))
        assert gpu_ctx.lde_columns(d_v, ncols, n, blow, d_c, d_l, want_split=True) == PROOF_SHAPES[shape]
    finally:
        for d in (d_v, d_c, d_l):
            gpu_ctx.free(d)


@pytest.mark.gpu
@pytest.mark.parametrize("np_", [4, 1])
@pytest.mark.parametrize("shape", sorted(PROOF_SHAPES))
def test_proofs_match_oracle_on_one_context(oracle, reference_proofs, pm_policy, shape, np_):
    """structured, unstructured, structured on one fresh context (the column map, the periodic
    tiles, the DEEP / OOD lists and the book of one proof must not leak into the next); then the
    host-trace entry point, whose LDE stays dense but whose DEEP and OOD take the lists; then the
    switch off, and on again."""
    log_n, blow = shape
    n = 1 << log_n
    ctx = zkl_hip.Context(0)
    try:
        dev = {}
        for kind, (seed, flags) in SEEDS.items():
            t, pi, w = zkl_hip.synth_vm_segment(seed, log_n, flags)
            d = ctx.alloc(C.sizeof(t))
            ctx.upload(d, t, C.sizeof(t))
            dev[kind] = (d, t, pi, w)
        per = ctx.scan_columns(dev["structured"][0], dev["structured"][3], n)
        assert {0, 32, 128, GEN} <= set(per)  # zero, periodic (both below n) and general columns

        def resident(kind):
            d, _, pi, w = dev[kind]
            assert ctx.prove_segment_device(d, w, n, pi, _options(w, log_n, blow, np_)) == \
                reference_proofs[log_n, blow, kind, np_], kind

        def host(kind):
            _, t, pi, w = dev[kind]
            assert ctx.prove_segment(t, w, n, pi, _options(w, log_n, blow, np_)) == \
                reference_proofs[log_n, blow, kind, np_], kind

        for kind in ("structured", "unstructured", "structured"):
            resident(kind)
        for kind in ("unstructured", "structured"):
            host(kind)
        resident("structured")  # after a dense LDE wrote every column
        with zkl_hip.column_structure(False):
            for kind in ("structured", "unstructured"):
                resident(kind)
                host(kind)
        resident("structured")  # and on again after the dense proofs
        for d, _, _, _ in dev.values():
            ctx.free(d)
    finally:
        ctx.close()
