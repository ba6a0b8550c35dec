"""Host traces as column pointers, classified while they are staged: the stage
entry point zkl_hip_lde_columns_host against the dense LDE of the uploaded matrix, the book of
what a context left zero, and whole proofs from columns against the flat and the device entry.

The dense path (lde_columns with the column-structure switch off) is pinned to the oracle by
tests/test_column_structure_lde.py; the device entry's proofs by tests/test_gpu_parity.py."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import zkl_hip

GEN = zkl_hip.COL_GENERAL
P_FIELD = 2**128 - 45 * 2**40 + 1
SEED = 0x5EED0001
# the segments of tests/test_host_columns_cpu.py: (log_n, flags) -> (zero, periodic, general)
SEGMENTS = {(5, 0): (169, 0, 35), (7, 1): (152, 37, 15), (8, 0): (145, 38, 21), (10, 3): (92, 29, 91),
            (8, 7): (148, 29, 42)}


def _col_buf(vals):
    return (C.c_uint8 * (16 * len(vals))).from_buffer_copy(b"".join(v.to_bytes(16, "little") for v in vals))


def _norm(per, n):
    """The scan reports a period up to min(128, n) even where it is n itself; the plan and the host
    classifier call that general."""
    return [x if (x in (0, GEN) or x < n) else GEN for x in per]


# ------------------------------------------------------------------ stage entry
def _periodic(rng, n, k):
    base = [rng.randrange(1, P_FIELD) for _ in range(k)]
    if k > 1:
        base[k // 2] = (base[0] + 1) % P_FIELD  # the smallest period is k itself
    return [base[i % k] for i in range(n)]


def _crafted(rng, n, kind):
    """(values or None for a NULL column, class the host must find)"""
    p = P_FIELD
    if kind == "null":
        return None, 0
    if kind == "zero":
        return [0] * n, 0
    if kind == "row0":
        return [5] + [0] * (n - 1), GEN
    if kind == "last":
        return [0] * (n - 1) + [1 << 64], GEN
    if kind == "const":
        return [rng.randrange(1, p)] * n, 1
    if kind == "general":
        return [rng.randrange(p) for _ in range(n)], GEN
    if kind == "hi2":  # differs only in the high word, period 2
        return [7 + ((i & 1) << 64) for i in range(n)], 2
    if kind == "late":  # periodic over rows 0..127, row 128 (the last row of a short column) differs
        col = _periodic(rng, n, 8)
        col[128 if n > 128 else n - 1] ^= 1
        return col, GEN
    if kind == "lastrow":  # periodic everywhere except the last row
        col = _periodic(rng, n, 2)
        col[n - 1] ^= 1 << 100
        return col, GEN
    k = int(kind)  # exact period k; a period that is not below n is general
    if k > n:
        return [rng.randrange(p) for _ in range(n)], GEN
    return _periodic(rng, n, k), (k if k < n else GEN)


MATRICES = {
    # 24 columns: every crafted kind, zero columns both as NULL and as arrays, first and last
    # column of several classes
    "mixed": ["null", "general", "const", "zero", "2", "general", "32", "null", "128", "row0", "zero", "last", "4",
              "8", "general", "16", "64", "hi2", "late", "lastrow", "null", "general", "128", "1"],
    "no_general": ["null", "const", "2", "zero", "4", "8", "16", "null", "hi2", "const", "zero", "2"] * 2,
    "only_general": ["general", "row0", "last", "late", "lastrow", "general"] * 4,
}


def _kinds(name, n):
    kinds = [("const" if k == "1" else k) for k in MATRICES[name]]
    if name == "no_general":  # periods that are not below n would be general
        kinds = [k if not k.isdigit() or int(k) < n else "const" for k in kinds]
    return kinds


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MATRICES))
@pytest.mark.parametrize("blow", [8, 16])
@pytest.mark.parametrize("n", [32, 64, 256, 1024])
def test_stage_entry_matches_dense(gpu_ctx, n, blow, name):
    """zkl_hip_lde_columns_host on separately allocated columns: the classes equal the device
    scan's of the uploaded matrix, coef / LDE / layout equal the dense stage's, with and without
    the split layout and with 1, 4 and the default number of general columns per chunk; the bytes
    that crossed the bus are those of the general columns and the periodic heads alone."""
    rng = random.Random(n * blow + len(name))
    made = [_crafted(rng, n, k) for k in _kinds(name, n)]
    ncols = len(made)
    want_per = [cls for _, cls in made]
    cols = [None if v is None else _col_buf(v) for v, _ in made]  # one allocation per column
    flat = b"".join(bytes(16 * n) if b is None else bytes(b) for b in cols)
    n_gen = want_per.count(GEN)
    n_per = sum(1 for x in want_per if x not in (0, GEN))
    if name == "no_general":
        assert n_gen == 0
    if name == "only_general":
        assert n_gen == ncols
    size = ncols * n * 16
    d_v, d_c, d_l = gpu_ctx.alloc(size), gpu_ctx.alloc(size), gpu_ctx.alloc(size * blow)
    try:
        gpu_ctx.upload(d_v, (C.c_uint8 * size).from_buffer_copy(flat), size)
        assert _norm(gpu_ctx.scan_columns(d_v, ncols, n), n) == want_per
        for want_split in (False, True):
            with zkl_hip.column_structure(False):
                sp0 = gpu_ctx.lde_columns(d_v, ncols, n, blow, d_c, d_l, want_split=want_split)
                coef0, lde0 = gpu_ctx.download(d_c, size), gpu_ctx.download(d_l, size * blow)
            for chunk in (1, 4, 0):
                gpu_ctx.set_upload_chunk_columns(chunk)
                try:
                    per, sp = gpu_ctx.lde_columns_host(cols, n, blow, d_c, d_l, want_split=want_split)
                finally:
                    gpu_ctx.set_upload_chunk_columns(0)
                assert per == want_per, (want_split, chunk)
                assert sp == sp0, (want_split, chunk)
                assert gpu_ctx.download(d_c, size) == coef0, (want_split, chunk)
                assert gpu_ctx.download(d_l, size * blow) == lde0, (want_split, chunk)
                st = gpu_ctx.upload_stats()
                assert (st["cols_zero"], st["cols_periodic"], st["cols_general"]) == \
                    (ncols - n_gen - n_per, n_per, n_gen)
                assert st["bytes_dma"] == (n_gen * n + n_per * min(128, n)) * 16
                assert st["bytes_pinned"] == st["bytes_dma"]
                assert st["chunks"] == (-(-n_gen // chunk) if chunk else min(1, n_gen))
    finally:
        for d in (d_v, d_c, d_l):
            gpu_ctx.free(d)


@pytest.mark.gpu
def test_stage_entry_switch_off_stages_every_column(gpu_ctx):
    """With the column-structure switch off every column is general: all of them are staged (a
    NULL column as zeros) and transformed."""
    n, blow = 64, 8
    rng = random.Random(64)
    made = [_crafted(rng, n, k) for k in _kinds("mixed", n)]
    ncols, size = len(made), len(made) * n * 16
    cols = [None if v is None else _col_buf(v) for v, _ in made]
    flat = b"".join(bytes(16 * n) if b is None else bytes(b) for b in cols)
    d_v, d_c, d_l = gpu_ctx.alloc(size), gpu_ctx.alloc(size), gpu_ctx.alloc(size * blow)
    try:
        gpu_ctx.upload(d_v, (C.c_uint8 * size).from_buffer_copy(flat), size)
        with zkl_hip.column_structure(False):
            gpu_ctx.lde_columns(d_v, ncols, n, blow, d_c, d_l)
            coef0, lde0 = gpu_ctx.download(d_c, size), gpu_ctx.download(d_l, size * blow)
            gpu_ctx.upload(d_c, (C.c_uint8 * size)(*([0xA5] * size)), size)
            per, _ = gpu_ctx.lde_columns_host(cols, n, blow, d_c, d_l)
            st = gpu_ctx.upload_stats()
        assert per == [GEN] * ncols
        assert (st["cols_zero"], st["cols_periodic"], st["cols_general"]) == (0, 0, ncols)
        assert st["bytes_dma"] == size
        assert gpu_ctx.download(d_c, size) == coef0
        assert gpu_ctx.download(d_l, size * blow) == lde0
    finally:
        for d in (d_v, d_c, d_l):
            gpu_ctx.free(d)


# ------------------------------------------------------------------ the book
@pytest.mark.gpu
def test_stage_book_across_class_changes():
    """One context, one buffer pair: matrix A (column 3 zero, column 5 periodic), then B (column 3
    general, column 5 zero), then A again; every result equals the dense one.  A slice wrongly
    remembered as zero, or a stale coefficient tail behind a periodic head, shows here."""
    n, blow, ncols = 256, 8, 8
    rng = random.Random(0xB00C5)
    kinds_a = ["general", "const", "general", "null", "32", "16", "zero", "general"]
    kinds_b = ["general", "const", "general", "general", "32", "zero", "2", "general"]
    size = ncols * n * 16
    ctx = zkl_hip.Context(0)
    try:
        mats = []
        for kinds in (kinds_a, kinds_b):
            made = [_crafted(rng, n, k) for k in kinds]
            cols = [None if v is None else _col_buf(v) for v, _ in made]
            flat = b"".join(bytes(16 * n) if b is None else bytes(b) for b in cols)
            mats.append((cols, flat, [cls for _, cls in made]))
        d_v, d_c0, d_l0 = ctx.alloc(size), ctx.alloc(size), ctx.alloc(size * blow)
        d_c, d_l = ctx.alloc(size), ctx.alloc(size * blow)
        dense = []
        with zkl_hip.column_structure(False):  # on a pair of its own: the pair under test is untouched
            for _, flat, _ in mats:
                ctx.upload(d_v, (C.c_uint8 * size).from_buffer_copy(flat), size)
                sp = ctx.lde_columns(d_v, ncols, n, blow, d_c0, d_l0, want_split=True)
                dense.append((sp, ctx.download(d_c0, size), ctx.download(d_l0, size * blow)))
        for step in (0, 1, 0, 1, 0):
            cols, _, want_per = mats[step]
            per, sp = ctx.lde_columns_host(cols, n, blow, d_c, d_l, want_split=True)
            assert per == want_per, step
            assert (sp, ctx.download(d_c, size), ctx.download(d_l, size * blow)) == dense[step], step
        for d in (d_v, d_c0, d_l0, d_c, d_l):
            ctx.free(d)
    finally:
        ctx.close()


# ------------------------------------------------------------------ proofs
def _segment(log_n, flags):
    """(flat trace, columns with every second zero column as None, pi, width, classes)"""
    n = 1 << log_n
    t, pi, w = zkl_hip.synth_vm_segment(SEED, log_n, flags)
    mat = np.frombuffer(t, dtype=np.uint64).reshape(w, n, 2)
    cols, zeros = [], 0
    for c in range(w):
        if not mat[c].any():
            zeros += 1
            if zeros % 2:
                cols.append(None)
                continue
        cols.append((C.c_uint8 * (n * 16)).from_buffer_copy(mat[c].tobytes()))
    per = zkl_hip.classify_columns(cols, n)
    return t, cols, pi, w, per


def _device_proof(ctx, t, w, n, pi, opts):
    d = ctx.alloc(w * n * 16)
    try:
        ctx.upload(d, t, w * n * 16)
        return ctx.prove_segment_device(d, w, n, pi, opts)
    finally:
        ctx.free(d)


def _staged_bytes(per, n):
    n_gen = per.count(GEN)
    n_per = sum(1 for x in per if x not in (0, GEN))
    return (n_gen * n + n_per * min(128, n)) * 16


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,flags", sorted(SEGMENTS))
def test_proofs_from_columns(gpu_ctx, log_n, flags):
    """Columns entry == flat entry == device entry, and the verifier accepts; with 4, 16 and the
    default number of general columns per chunk, with the column-structure switch off (W general
    columns staged) and with the preflight on."""
    n = 1 << log_n
    t, cols, pi, w, per = _segment(log_n, flags)
    zero, periodic, general = SEGMENTS[log_n, flags]
    assert (per.count(0), len(per) - per.count(0) - per.count(GEN), per.count(GEN)) == (zero, periodic, general)
    opts = zkl_hip.proof_options(w, n, queries=16, grind=4)
    want = _device_proof(gpu_ctx, t, w, n, pi, opts)
    zkl_hip.verify_segment(want, pi, opts)
    assert gpu_ctx.prove_segment(t, w, n, pi, opts) == want
    st = gpu_ctx.upload_stats()
    assert (st["cols_zero"], st["cols_periodic"], st["cols_general"]) == (zero, periodic, general)
    assert gpu_ctx.host_times()["upload"] > 0
    for chunk in (4, 16, 0):
        gpu_ctx.set_upload_chunk_columns(chunk)
        try:
            got = gpu_ctx.prove_segment_columns(cols, n, pi, opts)
        finally:
            gpu_ctx.set_upload_chunk_columns(0)
        assert got == want, chunk
        assert gpu_ctx.last_proof() == want
        st = gpu_ctx.upload_stats()
        assert (st["cols_zero"], st["cols_periodic"], st["cols_general"]) == (zero, periodic, general)
        assert st["bytes_dma"] == _staged_bytes(per, n)
        assert st["chunks"] == (-(-general // chunk) if chunk else 1)
    with zkl_hip.column_structure(False):
        assert gpu_ctx.prove_segment_columns(cols, n, pi, opts) == want
        st = gpu_ctx.upload_stats()
        assert (st["cols_zero"], st["cols_periodic"], st["cols_general"]) == (0, 0, w)
        assert st["bytes_dma"] == w * n * 16
        assert gpu_ctx.prove_segment(t, w, n, pi, opts) == want
    gpu_ctx.set_preflight(True)
    try:
        assert gpu_ctx.prove_segment_columns(cols, n, pi, opts) == want
        assert gpu_ctx.prove_segment(t, w, n, pi, opts) == want
    finally:
        gpu_ctx.set_preflight(False)
    assert gpu_ctx.prove_segment_columns(cols, n, pi, opts) == want


@pytest.mark.gpu
def test_proof_book_across_entries_and_segments():
    """One context alternating the columns, device and flat entries over two different segments
    (flags 0 and 1, n = 256): every proof equals the one a fresh context gives through the device
    entry.  The prover's book of zero slices, the column lists and the periodic tiles of one proof
    must not leak into the next, whichever entry made it."""
    log_n, n = 8, 256
    segs, want = {}, {}
    for flags in (0, 1):
        segs[flags] = _segment(log_n, flags)
        t, _, pi, w, _ = segs[flags]
        opts = zkl_hip.proof_options(w, n, queries=16, grind=4)
        fresh = zkl_hip.Context(0)
        try:
            want[flags] = _device_proof(fresh, t, w, n, pi, opts)
        finally:
            fresh.close()
    assert segs[0][4] != segs[1][4]  # the classes differ, column by column
    ctx = zkl_hip.Context(0)
    try:
        dev = {}
        for flags, (t, _, _, w, _) in segs.items():
            dev[flags] = ctx.alloc(w * n * 16)
            ctx.upload(dev[flags], t, w * n * 16)
        order = [("columns", 0), ("device", 1), ("flat", 0), ("columns", 1), ("columns", 0), ("flat", 1),
                 ("device", 0), ("columns", 1), ("device", 1), ("columns", 0)]
        for entry, flags in order:
            t, cols, pi, w, _ = segs[flags]
            opts = zkl_hip.proof_options(w, n, queries=16, grind=4)
            if entry == "columns":
                got = ctx.prove_segment_columns(cols, n, pi, opts)
            elif entry == "flat":
                got = ctx.prove_segment(t, w, n, pi, opts)
            else:
                got = ctx.prove_segment_device(dev[flags], w, n, pi, opts)
            assert got == want[flags], (entry, flags)
        for d in dev.values():
            ctx.free(d)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_two_contexts_prove_from_columns_at_once(gpu_ctx):
    """Two contexts, each with its own ring, workers and map buffers, proving from columns on two
    threads at the same time."""
    cases = []
    for log_n, flags in ((10, 3), (8, 7)):
        n = 1 << log_n
        t, cols, pi, w, _ = _segment(log_n, flags)
        opts = zkl_hip.proof_options(w, n, queries=16, grind=4)
        cases.append((cols, n, pi, opts, _device_proof(gpu_ctx, t, w, n, pi, opts)))
    ctxs = [zkl_hip.Context(0), zkl_hip.Context(0)]
    got = [[], []]
    errs = []

    def run(k):
        try:
            cols, n, pi, opts, _ = cases[k]
            ctxs[k].set_upload_chunk_columns(4)
            for _ in range(3):
                got[k].append(ctxs[k].prove_segment_columns(cols, n, pi, opts))
        except Exception as e:  # reported below, on the main thread
            errs.append(e)

    try:
        th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
    finally:
        for c in ctxs:
            c.close()
    assert not errs, errs
    for k in range(2):
        assert got[k] == [cases[k][4]] * 3


@pytest.mark.gpu
def test_headline_sized_proof_from_columns(gpu_ctx):
    """n = 2^16, W = 204, default chunking: 40 general columns of 1 MiB through the 16 MiB slots in
    three chunks; the bytes equal the device entry's and only the general columns and the periodic
    heads crossed the bus."""
    log_n, n = 16, 1 << 16
    t, cols, pi, w, per = _segment(log_n, 0)
    assert w == 204
    opts = zkl_hip.proof_options(w, n, queries=16, grind=4)
    want = _device_proof(gpu_ctx, t, w, n, pi, opts)
    assert gpu_ctx.prove_segment_columns(cols, n, pi, opts) == want
    st = gpu_ctx.upload_stats()
    assert (st["cols_zero"], st["cols_periodic"], st["cols_general"]) == (127, 37, 40)
    assert st["bytes_dma"] == (40 * n + 37 * 128) * 16 == _staged_bytes(per, n)
    assert st["bytes_pinned"] == st["bytes_dma"]
    assert st["chunks"] == 3


# ------------------------------------------------------------------ rejections
@pytest.mark.gpu
def test_rejections(gpu_ctx):
    """A NULL array and a wrong width are refused before any device work; a general column of a
    valid trace replaced by NULL fails the way any AIR-violating trace does, and the context proves
    correctly afterwards."""
    log_n, n = 8, 256
    t, cols, pi, w, per = _segment(log_n, 0)
    opts = zkl_hip.proof_options(w, n, queries=16, grind=4)
    lib = zkl_hip.load_library()
    out, ln = C.POINTER(C.c_uint8)(), C.c_size_t()
    assert lib.zkl_hip_prove_segment_columns(gpu_ctx.ptr, None, w, n, C.byref(pi), C.byref(opts), C.byref(out),
                                             C.byref(ln)) == -1
    with pytest.raises(zkl_hip.ZklError, match="width") as ei:
        gpu_ctx.prove_segment_columns(cols[:-1], n, pi, opts)
    assert ei.value.code == -1
    with pytest.raises(zkl_hip.ZklError, match="power of two") as ei:
        gpu_ctx.prove_segment_columns(cols, n - 1, pi, opts)
    assert ei.value.code == -1
    # a general column whose absence breaks a transition constraint in row 0 (checked on the host)
    victim = None
    for c in (c for c in range(w) if per[c] == GEN):
        cur, nxt = list(zkl_hip.trace_row(t, w, n, 0)), list(zkl_hip.trace_row(t, w, n, 1))
        cur[c] = nxt[c] = zkl_hip.F128(0, 0)
        if any(zkl_hip.eval_transition_row(w, n, pi, 0, cur, nxt)):
            victim = c
            break
    assert victim is not None
    broken = list(cols)
    broken[victim] = None
    with pytest.raises(zkl_hip.ZklError, match="degree too large"):
        gpu_ctx.prove_segment_columns(broken, n, pi, opts)
    with pytest.raises(zkl_hip.ZklError):
        gpu_ctx.last_proof()
    want = _device_proof(gpu_ctx, t, w, n, pi, opts)
    assert gpu_ctx.prove_segment_columns(cols, n, pi, opts) == want
