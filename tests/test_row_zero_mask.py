"""Zero mask of the prefix row kernel (DESIGN.md §4 "Row hash"): columns the plan marks zero are
not loaded in the blocks a partition still absorbs.  Every case compares all rows with the dense
kernel and with the mask switched off, and sampled rows with the oracle's row digest; the last test
proves one structured segment on one context with the mask off and on."""
import ctypes as C
import random

import numpy as np
import pytest

import zkl_hip

GEN = zkl_hip.COL_GENERAL


@pytest.fixture
def pm_policy(gpu_ctx):
    """Every Poseidon level of >= 32 states on the matrix-core permutation (the masked kernel is its
    row kernel); the default policy afterwards."""
    lib = zkl_hip.load_library()
    assert lib.zkl_hip_set_hash_policy(1, 32) == 0
    yield
    assert lib.zkl_hip_set_hash_policy(1, 1 << 14) == 0


def _fe_buf(vals):
    return (C.c_uint8 * (16 * len(vals))).from_buffer_copy(b"".join(v.to_bytes(16, "little") for v in vals))


def _column(rng, p, nrows, k):
    if k == GEN:
        return [rng.randrange(p) for _ in range(nrows)]
    if k == 0:
        return [0] * nrows
    base = [rng.randrange(1, p) for _ in range(k)]
    return [base[i % k] for i in range(nrows)]


def _crafted(rng, p, ncols, nrows, spec):
    """Column-major values and asserted row periods; spec: {column: period}, others random."""
    vals, per = [], []
    for c in range(ncols):
        k = spec.get(c, GEN)
        vals += _column(rng, p, nrows, k)
        per.append(k)
    return vals, per


def _row_digest(oracle, row, np_, rate=16):
    ncols = len(row)
    psize = ncols if np_ == 1 else max(-(-ncols // np_), rate)
    if psize == ncols:
        return oracle.hash_elements(row)
    return oracle.merge_many([oracle.hash_elements(row[c:c + psize]) for c in range(0, ncols, psize)])


def _check_rows(oracle, got, vals, ncols, nrows, np_, q, pos=lambda r: r):
    rows = sorted(set(list(range(0, nrows, 53)) + [0, 31, 32, q - 1, q, nrows - 1]))
    for r in rows:
        row = [vals[c * nrows + pos(r)] for c in range(ncols)]
        assert int.from_bytes(got[16 * r:16 * r + 16], "little") == _row_digest(oracle, row, np_), f"row {r}"


def _three_ways(ctx, d_m, d_o, ncols, nrows, np_, per, resumed, split=0):
    """Digests with the mask, with the mask off, and (natural layout) from the dense kernel."""
    with zkl_hip.row_zero_mask(True):
        assert ctx.hash_rows_periodic(d_m, ncols, nrows, np_, 16, per, d_o, split=split) == resumed
        got = ctx.download(d_o, nrows * 16)
    with zkl_hip.row_zero_mask(False):
        assert ctx.hash_rows_periodic(d_m, ncols, nrows, np_, 16, per, d_o, split=split) == resumed
        off = ctx.download(d_o, nrows * 16)
    with zkl_hip.column_structure(False):
        assert ctx.hash_rows_periodic(d_m, ncols, nrows, np_, 16, per, d_o, split=split) == 0
        dense = ctx.download(d_o, nrows * 16)
    assert got == off == dense
    if not split:
        ctx.hash_rows(d_m, ncols, nrows, np_, 16, d_o)
        assert ctx.download(d_o, nrows * 16) == got
    return got


def _masked_loads(per, np_, lead):
    """Column loads the mask removes, in the blocks still absorbed (pair j is sponge element j + 1)."""
    masks = zkl_hip.plan_row_zero_mask(per, np_, 16)
    psize = len(per) if np_ == 1 else max(-(-len(per) // np_), 16)
    n = 0
    for p, (even, odd) in enumerate(masks):
        ln = min(psize, len(per) - p * psize)
        for j in range((ln + 1) // 2):
            if (j + 1) // 10 >= lead[p]:
                n += ((even >> j) & 1) + (((odd >> j) & 1) if 2 * j + 1 < ln else 0)
    return n


def _bench_spec(rng):
    """204 columns in 4 partitions of 51 (blocks: partition columns 0..17, 18..37, 38..50).  The
    headline's lead (2, 0, 2, 0) plus zero columns where the kernel still absorbs."""
    spec = {c: rng.choice([0, 0, 1, 32, 128, 512]) for c in range(38)}
    spec[5], spec[20] = 512, 1
    spec.update({c: 0 for c in range(102, 140)})
    # partition 0, last block: a whole zero pair, a pair with only its even column zero, one with
    # only its odd column zero
    spec.update({38: 0, 39: 0, 40: 0, 43: 0})
    # partition 1 (lead 0): a zero pair in block 0, block 1 entirely zero, block 2 general
    spec.update({51 + 2: 0, 51 + 3: 0})
    spec.update({51 + c: 0 for c in range(18, 38)})
    spec[203] = 0  # partition 3: the lone 51st column
    return spec


@pytest.mark.gpu
def test_bench_pattern_with_zero_columns(oracle, gpu_ctx, pm_policy):
    rng = random.Random(0x20A5)
    ncols, nrows, np_ = 204, 4096, 4
    vals, per = _crafted(rng, oracle.P, ncols, nrows, _bench_spec(rng))
    assert zkl_hip.plan_row_prefix(per, 64 * nrows, 1, np_, 16) == ((2, 0, 2, 0), (512, None, 1, None))
    # 4 in partition 0, 22 in partition 1, none in partition 2 (its last block is general), 1 in partition 3
    assert _masked_loads(per, np_, (2, 0, 2, 0)) == 27
    d_m, d_o = gpu_ctx.alloc(16 * len(vals)), gpu_ctx.alloc(nrows * 16)
    try:
        for lone in (0, GEN):  # the lone last column zero, then general
            if lone == GEN:
                vals[203 * nrows:] = _column(rng, oracle.P, nrows, GEN)
                per[203] = GEN
                assert _masked_loads(per, np_, (2, 0, 2, 0)) == 26
            raw = _fe_buf(vals)
            gpu_ctx.upload(d_m, raw, len(raw))
            got = _three_ways(gpu_ctx, d_m, d_o, ncols, nrows, np_, per, 2)
            _check_rows(oracle, got, vals, ncols, nrows, np_, 512)
    finally:
        gpu_ctx.free(d_m)
        gpu_ctx.free(d_o)


# 51 x 1056, one partition, the last batch of rows partly filled: every column zero but a few
ONE_PARTITION = {
    # three general columns in three blocks and a constant in block 0: lead 0, so the plan resumes
    # nothing and the dense kernel runs (the masked kernel for such plans is not built)
    "lead0": ({c: 0 for c in range(51)} | {4: 1, 7: GEN, 25: GEN, 45: GEN}, 0, 1),
    # the same with block 0 structured: resumed from the table, blocks 1 and 2 masked
    "lead1": ({c: 0 for c in range(51)} | {4: 1, 9: 8, 25: GEN, 44: GEN, 45: GEN}, 1, 8),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ONE_PARTITION))
def test_one_partition_mostly_zero(oracle, gpu_ctx, pm_policy, case):
    spec, resumed, q = ONE_PARTITION[case]
    rng = random.Random(sum(map(ord, case)))
    ncols, nrows, np_ = 51, 1056, 1
    vals, per = _crafted(rng, oracle.P, ncols, nrows, spec)
    assert zkl_hip.plan_row_prefix(per, 64 * 4096, 1, np_, 16)[0] == (resumed,)
    assert _masked_loads(per, np_, (resumed,)) == (47 if case == "lead0" else 30)
    raw = _fe_buf(vals)
    d_m, d_o = gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(nrows * 16)
    try:
        gpu_ctx.upload(d_m, raw, len(raw))
        got = _three_ways(gpu_ctx, d_m, d_o, ncols, nrows, np_, per, resumed)
    finally:
        gpu_ctx.free(d_m)
        gpu_ctx.free(d_o)
    _check_rows(oracle, got, vals, ncols, nrows, np_, max(q, 2))


def _lde_pos(r, n_rows):
    """kernels.h lde_pos: position of natural row r in the split layout."""
    log_s = n_rows.bit_length() - 1 - 8
    s = 1 << log_s
    big_l, t = r & (s - 1), r >> log_s
    lo = big_l & 7
    return (big_l - lo) + (lo >> 1) + ((t & 1) << 2) + (((t >> 1) + ((lo & 1) << 7)) << log_s)


@pytest.mark.gpu
def test_zero_columns_in_the_split_layout(oracle, gpu_ctx, pm_policy):
    """204 x 256 trace, blowup 8, through the LDE stage in the split layout; zero columns after the
    lead blocks of the resumed partitions and in the dense ones."""
    rng = random.Random(0x5B18)
    p, ncols, n, blow, np_ = oracle.P, 204, 256, 8, 4
    nrows = n * blow
    spec = {c: rng.choice([0, 1, 2, 4]) for c in range(18)}
    spec[2], spec[9] = 4, 1
    spec.update({c: 0 for c in range(102, 120)})
    spec.update({c: 0 for c in (20, 21, 22, 25, 40, 50, 60, 61, 75, 120, 121, 130, 151, 152, 203)})
    vals, per = _crafted(rng, p, ncols, n, spec)
    raw = _fe_buf(vals)
    d_v, d_c, d_l, d_o = (gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(len(raw) * blow),
                          gpu_ctx.alloc(nrows * 16))
    try:
        gpu_ctx.upload(d_v, raw, len(raw))
        assert gpu_ctx.scan_columns(d_v, ncols, n) == per
        assert gpu_ctx.lde_columns(d_v, ncols, n, blow, d_c, d_l, want_split=True) == 1
        lde = gpu_ctx.download(d_l, len(raw) * blow)
        asserted = [(k * blow if k > 1 else k) if k != GEN else GEN for k in per]
        assert zkl_hip.plan_row_prefix(asserted, nrows, 1, np_, 16)[0] == (1, 0, 1, 0)
        assert _masked_loads(asserted, np_, (1, 0, 1, 0)) == 15
        got = _three_ways(gpu_ctx, d_l, d_o, ncols, nrows, np_, asserted, 2, split=1)
    finally:
        for d in (d_v, d_c, d_l, d_o):
            gpu_ctx.free(d)
    cols = np.frombuffer(lde, dtype=np.uint64).reshape(ncols, nrows, 2)
    nat = cols[:, [_lde_pos(r, nrows) for r in range(nrows)], :]
    for c, k in spec.items():
        if k == 0:
            assert not nat[c].any(), c
    ints = [int(nat[c, r, 0]) | (int(nat[c, r, 1]) << 64) for c in range(ncols) for r in range(nrows)]
    _check_rows(oracle, got, ints, ncols, nrows, np_, 32)


@pytest.mark.gpu
def test_partition_over_the_mask_capacity(oracle, gpu_ctx, pm_policy):
    """One partition of 140 columns is 70 pairs, more than a mask holds: the plan carries an empty
    mask, the resumed kernel loads every column, zero ones included."""
    rng = random.Random(0x0CA9)
    ncols, nrows, np_ = 140, 160, 1
    spec = {c: 0 for c in range(18)} | {3: 1, 30: 0, 31: 0, 64: 0, 99: 0, 138: 0, 139: 0}
    vals, per = _crafted(rng, oracle.P, ncols, nrows, spec)
    assert zkl_hip.plan_row_prefix(per, 64 * 4096, 1, np_, 16) == ((1,), (1,))
    assert zkl_hip.plan_row_zero_mask(per, np_, 16) == ((0, 0),)
    raw = _fe_buf(vals)
    d_m, d_o = gpu_ctx.alloc(len(raw)), gpu_ctx.alloc(nrows * 16)
    try:
        gpu_ctx.upload(d_m, raw, len(raw))
        got = _three_ways(gpu_ctx, d_m, d_o, ncols, nrows, np_, per, 1)
    finally:
        gpu_ctx.free(d_m)
        gpu_ctx.free(d_o)
    _check_rows(oracle, got, vals, ncols, nrows, np_, 2)


LOG_N, QUERIES, BLOWUP, GRIND = 10, 32, 16, 4


@pytest.mark.gpu
def test_proofs_with_the_mask_off_and_on(gpu_ctx, pm_policy):
    """Proofs of one structured segment on a fresh context, mask off then on: the later ones find the
    zero-fill book filled by the first.  The bytes are those of the dense path (which
    tests/test_column_structure.py holds against the oracle)."""
    n = 1 << LOG_N
    t, pi, w = zkl_hip.synth_vm_segment(0x5EED0001, LOG_N, 0)
    o = zkl_hip.proof_options(w, n, queries=QUERIES, blowup=BLOWUP, grind=GRIND)
    o.num_partitions, o.hash_rate = 4, 16
    ctx = zkl_hip.Context(0)
    try:
        d = ctx.alloc(C.sizeof(t))
        ctx.upload(d, t, C.sizeof(t))
        with zkl_hip.row_zero_mask(False):
            off = ctx.prove_segment_device(d, w, n, pi, o)
        with zkl_hip.row_zero_mask(True):
            on = ctx.prove_segment_device(d, w, n, pi, o)
            again = ctx.prove_segment_device(d, w, n, pi, o)
        with zkl_hip.column_structure(False):
            dense = ctx.prove_segment_device(d, w, n, pi, o)
        ctx.free(d)
    finally:
        ctx.close()
    assert off == on == again == dense
