"""The matrix-core Poseidon round after its carry rewrite, on the device: the permutation stage
entry of both matrix-core forms on states made of the field's corner elements, and a row hash
whose sponge absorbs a second block, so that the first cube after an absorb (mont_cube130, as
before) runs next to the round loop's mont_cube130_chain.  Against the oracle."""
import ctypes as C
import random

import pytest

pytestmark = pytest.mark.gpu


def _fe_buf(vals):
    return (C.c_uint8 * (16 * len(vals))).from_buffer_copy(b"".join(v.to_bytes(16, "little") for v in vals))


def _corners(P):
    return [0, 1, P - 1, 1 << 127, ((1 << 128) - 1) % P]


@pytest.mark.parametrize("engine", [1, 2])
def test_permute_corner_states(oracle, gpu_ctx, engine):
    """64 states (two batches of the 32-state form, four of the 16-state form): each corner in
    every element, each corner alone among zeros and among p - 1, and random mixes of corners."""
    P = oracle.P
    corners = _corners(P)
    rng = random.Random(1000 + engine)
    states = [[e] * 12 for e in corners]
    for e in corners[1:]:
        k = rng.randrange(12)
        states.append([e if j == k else 0 for j in range(12)])
        states.append([e if j == k else P - 1 for j in range(12)])
    states += [[rng.choice(corners) for _ in range(12)] for _ in range(64 - len(states))]
    assert len(states) == 64
    flat = [x for s in states for x in s]
    d = gpu_ctx.alloc(16 * len(flat))
    gpu_ctx.upload(d, _fe_buf(flat), 16 * len(flat))
    gpu_ctx.poseidon_permute(d, 64, engine)
    got = gpu_ctx.download(d, 16 * len(flat))
    gpu_ctx.free(d)
    for i, s in enumerate(states):
        have = [int.from_bytes(got[16 * (12 * i + j):16 * (12 * i + j) + 16], "little") for j in range(12)]
        assert have == oracle.permute(s), f"state {i}"


def test_row_hash_two_absorb_blocks(oracle, gpu_ctx):
    """64 rows x 23 columns, one partition: 12 folded pairs, i.e. two absorb blocks per row, on the
    matrix-core row kernel; rows of corners and random rows."""
    import zkl_hip
    lib = zkl_hip.load_library()
    P = oracle.P
    corners = _corners(P)
    rng = random.Random(23)
    ncols, nrows = 23, 64
    rows = [[e] * ncols for e in corners]
    rows += [[rng.choice(corners) for _ in range(ncols)] for _ in range(27)]
    rows += [[rng.randrange(P) for _ in range(ncols)] for _ in range(nrows - len(rows))]
    vals = [rows[r][c] for c in range(ncols) for r in range(nrows)]  # column-major
    raw = _fe_buf(vals)
    d_m = gpu_ctx.alloc(len(raw))
    d_o = gpu_ctx.alloc(nrows * 16)
    gpu_ctx.upload(d_m, raw, len(raw))
    assert lib.zkl_hip_set_hash_policy(1, 32) == 0  # rows of >= 32 states go to the matrix cores
    try:
        gpu_ctx.hash_rows(d_m, ncols, nrows, 1, 16, d_o)
    finally:
        assert lib.zkl_hip_set_hash_policy(1, 1 << 14) == 0
    got = gpu_ctx.download(d_o, nrows * 16)
    for d in (d_m, d_o):
        gpu_ctx.free(d)
    for r in range(nrows):
        assert int.from_bytes(got[16 * r:16 * r + 16], "little") == oracle.hash_elements(rows[r]), f"row {r}"
