"""Column structure: the exact column scan, the host plan of the row hash's prefix
skip, the prefix row hash against the oracle's hash_elements / merge_many, and whole proofs of
structured and unstructured segments against the oracle's proofs.

The row-hash stage takes periods its caller asserts, so those matrices are crafted; the scan and
the proofs find the structure themselves.  Reference proofs are computed once per module."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import zkl_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = zkl_hip.COL_GENERAL
P_MAX = 128


def _columns(trace, w, n):
    """(w, n, 2) uint64 view of a column-major F128 trace (lo, hi)."""
    return np.frombuffer(trace, dtype=np.uint64).reshape(w, n, 2)


def _periods(cols, p_max=P_MAX):
    """numpy restatement of the scan: 0 all-zero, smallest power-of-two period <= p_max, GEN."""
    out = []
    for col in cols:
        if not col.any():
            out.append(0)
            continue
        per, p = GEN, 1
        while p <= min(p_max, col.shape[0]):
            if (col.reshape(-1, p, 2) == col[:p]).all():
                per = p
                break
            p *= 2
        out.append(per)
    return out


def _lde_pos(r, n_rows):
    """kernels.h lde_pos: position of natural row r in the split layout."""
    log_s = n_rows.bit_length() - 1 - 8
    s = 1 << log_s
    big_l, t = r & (s - 1), r >> log_s
    lo = big_l & 7
    return (big_l - lo) + (lo >> 1) + ((t & 1) << 2) + (((t >> 1) + ((lo & 1) << 7)) << log_s)


def _fe_buf(vals):
    return (C.c_uint8 * (16 * len(vals))).from_buffer_copy(b"".join(v.to_bytes(16, "little") for v in vals))


def _row_digest(oracle, row, np_, rate=16):
    ncols = len(row)
    psize = ncols
    if np_ > 1:
        psize = max(-(-ncols // np_), rate)
    if psize == ncols:
        return oracle.hash_elements(row)
    return oracle.merge_many([oracle.hash_elements(row[c:c + psize]) for c in range(0, ncols, psize)])


@pytest.fixture
def pm_policy(gpu_ctx):
    """Every Poseidon level of >= 32 states on the matrix-core permutation (the prefix skip lives in
    its row kernel); the default policy afterwards."""
    lib = zkl_hip.load_library()
    assert lib.zkl_hip_set_hash_policy(1, 32) == 0
    yield
    assert lib.zkl_hip_set_hash_policy(1, 1 << 14) == 0


# ------------------------------------------------------------------ CPU: the plan
def _oracle_periods(oracle, seed, log_n, flags=0):
    t, _, w = oracle.synth_segment(seed, log_n, flags)
    return _periods(_columns(t, w, 1 << log_n))


def test_plan_of_the_bench_segment(oracle):
    """synth_vm_segment(0x5EED0001, 10): its column periods are those of the 2^16-row headline
    segment (the VM layout's zero feature columns and per-level selectors), planned here at the
    headline LDE (2^20 rows, blowup 16)."""
    per = _oracle_periods(oracle, 0x5EED0001, 10)
    assert len(per) == 204
    assert zkl_hip.plan_row_prefix(per, 1 << 20, 16, 4, 16) == ((2, 0, 2, 0), (512, None, 1, None))
    # one partition: 204 columns = 103 sponge elements = 11 blocks, the first two structured
    assert zkl_hip.plan_row_prefix(per, 1 << 20, 16, 1, 16) == ((2,), (512,))
    # q = 512 > 2^14 / 64: that partition keeps the dense path, the all-zero one (q = 1) does not
    assert zkl_hip.plan_row_prefix(per, 1 << 14, 16, 4, 16) == ((0, 0, 2, 0), (None, None, 1, None))
    assert zkl_hip.plan_row_prefix(per, 1 << 15, 16, 4, 16)[0] == (2, 0, 2, 0)  # 512 == 2^15 / 64


def _plan_ref(per, n_lde, blowup, np_, rate=16):
    """The plan rule restated: per partition, leading blocks of 10 sponge elements (the domain
    element, then one per folded column pair) whose columns are all structured; q = blowup * the
    largest period among them, 1 when none exceeds 1; dropped when q > n_lde / 64."""
    ncols = len(per)
    psize = ncols if np_ == 1 else max(-(-ncols // np_), rate)
    lead, qs = [], []
    for c0 in range(0, ncols, psize):
        cols = per[c0:c0 + psize]
        total = (len(cols) + 1) // 2 + 1
        k, pmax = 0, 1
        for b0 in range(0, total, 10):
            blk = [cols[c] for i in range(max(b0, 1), min(b0 + 10, total)) for c in (2 * i - 2, 2 * i - 1) if c < len(cols)]
            if any(x == GEN for x in blk):
                break
            k, pmax = k + 1, max([pmax] + blk)
        q = blowup * pmax if pmax > 1 else 1
        ok = k > 0 and q <= n_lde // 64
        lead.append(k if ok else 0)
        qs.append(q if ok else None)
    return tuple(lead), tuple(qs)


def _rollup_periods(oracle, r_end):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "programs.json")))["rollup-bench"]
    ops = [zkl_hip.op(k, **f) for k, f in g["ops"]]
    ma = [(tg, bytes.fromhex(b)) for tg, b in g["cli"]["main_args"]]
    arr = (zkl_hip.ZklOp * len(ops))(*ops)
    rc, t, _, w, _, _ = oracle.build_segment_trace(arr, bytes.fromhex(g["program_id"]), 0, r_end,
                                                   secret_args=g["cli"]["secret_u64"], main_args=zkl_hip._vm_args(ma))
    assert rc == 0 and w == 212
    return _periods(_columns(t, w, r_end))


def test_plan_finds_nothing_in_sponge_and_rollup_segments(oracle):
    """Segments with sponge ops have general columns in every partition's first block: lead
    (0, 0, 0, 0), so they run the dense kernels.  That holds for the synthetic flags = 1 segment
    and for rollup-bench as one 65,536-row segment (212 columns: 75 zero, 29 of period 32, 108
    general).  Its first 4,096 rows alone are a different trace: the program has not reached
    its sponge and RAM ops there (116 zero columns, 31 of period 32, 65 general), and the rule gives
    that segment (2, 0, 2, 0) like a VM-only one; the plan is checked against the rule restated
    above rather than against (0, 0, 0, 0)."""
    per = _oracle_periods(oracle, 0x5EED0001, 10, flags=1)
    assert zkl_hip.plan_row_prefix(per, 1 << 20, 16, 4, 16) == ((0, 0, 0, 0), (None,) * 4)
    per = _rollup_periods(oracle, 65536)
    assert zkl_hip.plan_row_prefix(per, 1 << 20, 16, 4, 16) == ((0, 0, 0, 0), (None,) * 4)
    per = _rollup_periods(oracle, 4096)
    assert zkl_hip.plan_row_prefix(per, 1 << 20, 16, 4, 16) == _plan_ref(per, 1 << 20, 16, 4) == \
        ((2, 0, 2, 0), (512, None, 1, None))


def test_plan_matches_the_rule_restated(oracle):
    rng = random.Random(77)
    cases = [_oracle_periods(oracle, 0x5EED0001, 10), _oracle_periods(oracle, 0x5EED0002, 10, 1)]
    for _ in range(40):
        w = rng.choice([7, 33, 51, 102, 204, 212])
        cases.append([rng.choice([0, 0, 0, 1, 2, 32, 128, GEN]) if rng.random() < 0.9 else GEN for _ in range(w)])
    for per in cases:
        for np_ in (1, 2, 4, 9):
            for n_lde in (1 << 11, 1 << 14, 1 << 20):
                assert zkl_hip.plan_row_prefix(per, n_lde, 16, np_, 16) == _plan_ref(per, n_lde, 16, np_), (per, np_, n_lde)


def test_plan_block_boundaries():
    """Block k of a partition holds sponge elements 10k..10k+9: the domain element, then one per
    folded column pair, so blocks cover columns 0..17, 18..37, 38..57, ...  One general column
    ends the prefix at its block; periods that are no power of two count as general."""
    per = [0] * 51
    assert zkl_hip.plan_row_prefix(per, 4096, 1, 1, 16) == ((3,), (1,))
    for bad, lead in ((0, 0), (17, 0), (18, 1), (37, 1), (38, 2), (50, 2)):
        p2 = list(per)
        p2[bad] = GEN
        assert zkl_hip.plan_row_prefix(p2, 4096, 1, 1, 16)[0] == (lead,), bad
    p2 = list(per)
    p2[3] = 1   # constant: q stays 1
    p2[20] = 8  # second block: q = blowup * 8
    assert zkl_hip.plan_row_prefix(p2, 1 << 16, 16, 1, 16) == ((3,), (128,))
    p2[40] = 24
    assert zkl_hip.plan_row_prefix(p2, 1 << 16, 16, 1, 16)[0] == (2,)
    # more than 9 partitions (merge_many over two blocks) keep the dense path
    assert zkl_hip.plan_row_prefix([0] * 256, 1 << 16, 16, 16, 16)[0] == (0,) * 16


# ------------------------------------------------------------------ GPU: the scan
@pytest.mark.gpu
def test_scan_matches_numpy(oracle, gpu_ctx):
    rng = random.Random(0xC01)
    p, n, w = oracle.P, 1024, 24

    def periodic(k):
        base = [rng.randrange(p) for _ in range(k)]
        return [base[i % k] for i in range(n)]

    last_only = [0] * (n - 1) + [5]
    almost32 = periodic(32)
    almost32[777] = (almost32[777] + 1) % p
    cols = [[0] * n, [0] * n, [p - 1] * n, periodic(2), periodic(32), periodic(128), periodic(256),
            [rng.randrange(p) for _ in range(n)], last_only, almost32,
            [1] * n, periodic(4), periodic(8), periodic(16), periodic(64), periodic(512),
            [0] * 128 + [1] + [0] * (n - 129),        # first reference window all zero, then a one
            [7] * 512 + [8] * 512,                    # constant in each half
            periodic(2)[:-1] + [3], [0] * n, periodic(128)[:1000] + [rng.randrange(p) for _ in range(24)],
            [1 << 127] * n, [rng.randrange(p) for _ in range(n)], [0] * n]
    assert len(cols) == w
    flat = [v for c in cols for v in c]
    want = _periods(_columns(bytes(_fe_buf(flat)), w, n))
    assert want[:10] == [0, 0, 1, 2, 32, 128, GEN, GEN, GEN, GEN]
    d = gpu_ctx.alloc(16 * len(flat))
    gpu_ctx.upload(d, _fe_buf(flat), 16 * len(flat))
    got = gpu_ctx.scan_columns(d, w, n)
    gpu_ctx.free(d)
    assert got == want


# ------------------------------------------------------------------ GPU: the prefix row hash
def _crafted(rng, p, ncols, nrows, spec):
    """Column-major values and asserted row periods; spec: {column: period}, others random."""
    vals, per = [], []
    for c in range(ncols):
        k = spec.get(c, GEN)
        if k == GEN:
            col = [rng.randrange(p) for _ in range(nrows)]
        elif k == 0:
            col = [0] * nrows
        else:
            base = [rng.randrange(1, p) for _ in range(k)]
            col = [base[i % k] for i in range(nrows)]
        vals += col
        per.append(k)
    return vals, per


def _check_rows(oracle, got, vals, ncols, nrows, np_, q, pos=lambda r: r):
    rows = sorted(set(list(range(0, nrows, 53)) + [0, 31, 32, q - 1, q, nrows - 1]))
    for r in rows:
        row = [vals[c * nrows + pos(r)] for c in range(ncols)]
        assert int.from_bytes(got[16 * r:16 * r + 16], "little") == _row_digest(oracle, row, np_), f"row {r}"


def _bench_pattern(rng):
    """Partition 0: columns 0..37 zero / constant / periodic up to 512 rows; partition 2: columns
    102..139 zero; the rest general (the headline segment's lead (2, 0, 2, 0), q (512, -, 1, -))."""
    spec = {c: rng.choice([0, 0, 1, 32, 128, 512]) for c in range(38)}
    spec[5], spec[20] = 512, 1
    spec.update({c: 0 for c in range(102, 140)})
    return spec


HASH_CASES = {
    "bench_4096x204": (204, 4096, 4, _bench_pattern, 2, 512),
    # the whole partition structured: the digest comes from the table; 1056 rows leave the last
    # block of waves partly filled
    "all_structured_1056x51": (51, 1056, 1, lambda rng: {c: rng.choice([0, 1, 2, 8, 32]) for c in range(50)} | {50: 32},
                               1, 32),
    # a non-zero constant among zeros: q = 1, one table entry
    "constant_2048x102": (102, 2048, 2, lambda rng: {c: 0 for c in range(18)} | {4: 1, 11: 1}, 1, 1),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(HASH_CASES))
def test_prefix_row_hash_matches_oracle(oracle, gpu_ctx, pm_policy, case):
    ncols, nrows, np_, make, resumed, q = HASH_CASES[case]
    rng = random.Random(sum(map(ord, case)))
    vals, per = _crafted(rng, oracle.P, ncols, nrows, make(rng))
    lead, qs = zkl_hip.plan_row_prefix(per, 64 * 4096, 1, np_, 16)  # the pattern's plan, table cost aside
    assert sum(1 for x in lead if x) == resumed and max(x for x in qs if x) == q
    raw = _fe_buf(vals)
    d_m, d_o = gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(nrows * 16)
    gpu_ctx.upload(d_m, raw, len(raw))
    assert gpu_ctx.hash_rows_periodic(d_m, ncols, nrows, np_, 16, per, d_o) == resumed
    got = gpu_ctx.download(d_o, nrows * 16)
    with zkl_hip.column_structure(False):
        assert gpu_ctx.hash_rows_periodic(d_m, ncols, nrows, np_, 16, per, d_o) == 0
        off = gpu_ctx.download(d_o, nrows * 16)
    gpu_ctx.hash_rows(d_m, ncols, nrows, np_, 16, d_o)
    dense = gpu_ctx.download(d_o, nrows * 16)
    gpu_ctx.free(d_m)
    gpu_ctx.free(d_o)
    _check_rows(oracle, got, vals, ncols, nrows, np_, q)
    assert got == off == dense  # every row, against the dense kernels


@pytest.mark.gpu
def test_prefix_row_hash_in_the_split_layout(oracle, gpu_ctx, pm_policy):
    """204 x 256 trace, blowup 8, through the LDE stage in the split layout: a column of row
    period P has LDE row period 8 P in natural order (a constant stays constant, zero stays zero),
    and the row kernel, which walks positions, must index the table by lde_row(position) mod q."""
    rng = random.Random(0x5B17)
    p, ncols, n, blow, np_ = oracle.P, 204, 256, 8, 4
    nrows = n * blow
    spec = {c: rng.choice([0, 1, 2, 4]) for c in range(18)}
    spec[2], spec[9] = 4, 1
    spec.update({c: 0 for c in range(102, 120)})
    vals, per = _crafted(rng, p, ncols, n, spec)
    raw = _fe_buf(vals)
    d_v, d_c, d_l, d_o = (gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(len(raw) * blow),
                          gpu_ctx.alloc(nrows * 16))
    gpu_ctx.upload(d_v, raw, len(raw))
    assert gpu_ctx.scan_columns(d_v, ncols, n) == per
    assert gpu_ctx.lde_columns(d_v, ncols, n, blow, d_c, d_l, want_split=True) == 1
    lde = gpu_ctx.download(d_l, len(raw) * blow)
    with zkl_hip.column_structure(False):  # every column transformed: the same LDE
        assert gpu_ctx.lde_columns(d_v, ncols, n, blow, d_c, d_l, want_split=True) == 1
        assert gpu_ctx.download(d_l, len(raw) * blow) == lde
    cols = _columns(lde, ncols, nrows)
    nat = cols[:, [_lde_pos(r, nrows) for r in range(nrows)], :]
    row_per = _periods(nat, p_max=nrows)
    for c, k in spec.items():
        assert row_per[c] == (k * blow if k > 1 else k), c
    asserted = [(k * blow if k > 1 else k) if k != GEN else GEN for k in per]
    assert gpu_ctx.hash_rows_periodic(d_l, ncols, nrows, np_, 16, asserted, d_o, split=1) == 2
    got = gpu_ctx.download(d_o, nrows * 16)
    with zkl_hip.column_structure(False):
        assert gpu_ctx.hash_rows_periodic(d_l, ncols, nrows, np_, 16, asserted, d_o, split=1) == 0
        assert gpu_ctx.download(d_o, nrows * 16) == got
    for d in (d_v, d_c, d_l, d_o):
        gpu_ctx.free(d)
    ints = [int(nat[c, r, 0]) | (int(nat[c, r, 1]) << 64) for c in range(ncols) for r in range(nrows)]
    _check_rows(oracle, got, ints, ncols, nrows, np_, 32)


# ------------------------------------------------------------------ GPU: whole proofs
LOG_N, QUERIES, BLOWUP, GRIND = 10, 32, 16, 4
SEEDS = {"structured": (0x5EED0001, 0), "unstructured": (0x5EED0001, 1)}


def _options(w, np_):
    o = zkl_hip.proof_options(w, 1 << LOG_N, queries=QUERIES, blowup=BLOWUP, grind=GRIND)
    o.num_partitions, o.hash_rate = np_, 16
    return o


@pytest.fixture(scope="module")
def reference_proofs(oracle):
    """The oracle's proofs of both segments at 4 and 1 partitions, computed once."""
    out = {}
    oracle.set_threads(16)
    try:
        for kind, (seed, flags) in SEEDS.items():
            ot, opi, w = oracle.synth_segment(seed, LOG_N, flags)
            for np_ in (4, 1):
                o = _options(w, np_)
                oo = oracle.ProofOptions(*[getattr(o, f) for f, _ in o._fields_])
                out[kind, np_] = oracle.prove(ot, w, 1 << LOG_N, opi, oo)
    finally:
        oracle.set_threads(1)
    return out


def _segment(kind):
    seed, flags = SEEDS[kind]
    return zkl_hip.synth_vm_segment(seed, LOG_N, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("np_", [4, 1])
def test_proofs_match_oracle_on_one_context(oracle, reference_proofs, pm_policy, np_):
    """structured, unstructured, structured on one fresh context: the zero-fill bookkeeping and
    the prefix table of one proof must not leak into the next; then the same with the switch
    off, and through the host-trace entry point."""
    ctx = zkl_hip.Context(0)
    try:
        n = 1 << LOG_N
        dev = {}
        for kind in SEEDS:
            t, pi, w = _segment(kind)
            d = ctx.alloc(C.sizeof(t))
            ctx.upload(d, t, C.sizeof(t))
            dev[kind] = (d, t, pi, w)
        for kind in ("structured", "unstructured", "structured"):
            d, t, pi, w = dev[kind]
            assert ctx.prove_segment_device(d, w, n, pi, _options(w, np_)) == reference_proofs[kind, np_], kind
        for kind in ("unstructured", "structured"):  # host trace: scanned behind its upload
            d, t, pi, w = dev[kind]
            assert ctx.prove_segment(t, w, n, pi, _options(w, np_)) == reference_proofs[kind, np_], kind
        d, t, pi, w = dev["structured"]  # resident again after a dense LDE wrote every column
        assert ctx.prove_segment_device(d, w, n, pi, _options(w, np_)) == reference_proofs["structured", np_]
        with zkl_hip.column_structure(False):
            for kind in ("structured", "unstructured"):
                d, t, pi, w = dev[kind]
                assert ctx.prove_segment_device(d, w, n, pi, _options(w, np_)) == reference_proofs[kind, np_], kind
                assert ctx.prove_segment(t, w, n, pi, _options(w, np_)) == reference_proofs[kind, np_], kind
        d, t, pi, w = dev["structured"]  # and on again after the dense proofs
        assert ctx.prove_segment_device(d, w, n, pi, _options(w, np_)) == reference_proofs["structured", np_]
        for d, _, _, _ in dev.values():
            ctx.free(d)
    finally:
        ctx.close()


def test_structured_segment_has_a_prefix_at_the_proof_shape(oracle):
    """The proof tests above do exercise the skip: at 2^10 rows the structured segment resumes its
    all-zero partition (q = 1; q = 512 exceeds 2^14 / 64), the sponge segment nothing."""
    per = _oracle_periods(oracle, *[SEEDS["structured"][0], LOG_N, 0])
    assert zkl_hip.plan_row_prefix(per, BLOWUP << LOG_N, BLOWUP, 4, 16)[0] == (0, 0, 2, 0)
    assert zkl_hip.plan_row_prefix(per, BLOWUP << LOG_N, BLOWUP, 1, 16)[0] == (0,)
    per = _oracle_periods(oracle, *[SEEDS["unstructured"][0], LOG_N, 1])
    assert zkl_hip.plan_row_prefix(per, BLOWUP << LOG_N, BLOWUP, 4, 16)[0] == (0, 0, 0, 0)
