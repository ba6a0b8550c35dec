"""Device ZlAggAir prover (csrc/agg.hip): with a context the aggregation proof's
arrays -- trace LDE, commitments, constraint composition, DEEP, FRI, in the base field or the
quadratic extension -- are computed on the device; every artifact and every stage-entry proof is
byte for byte what the host backend writes."""
import random

import pytest

from test_batch_verify import PROGRAM, chain_steps
from test_gpu_batch_verify import AGG_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    import zkl_hip
    return zkl_hip


def random_trace_bytes(seed, n):
    """31 x n canonical elements, column-major (top byte of each clear: below the modulus)."""
    rng = random.Random(seed)
    return b"".join(rng.getrandbits(120).to_bytes(16, "little") for _ in range(31 * n))


PI_ELEMENTS = [(0x9E3779B97F4A7C15 * (k + 1)) % (1 << 100) for k in range(33)]

# n, blowup, min_security_bits (128: fe2, 64: fe), queries, grind.  N = 16 is below a
# wavefront with 2 FRI layers; 8 .. 16 rows are below what the segment prover's transforms take;
# 512 x 16 is the 256-child shape; 256 x 128 the largest blowup; 8192 x 2 the largest n, whose
# 2^14 LDE rows are also the first size the matrix-core row hash takes.  queries 64 on N = 16
# leaves far fewer unique positions than draws (dedup, shared openings).
TRACE_CASES = [
    (8, 2, 128, 64, 0),
    (8, 16, 64, 16, 8),
    (16, 8, 128, 16, 0),
    (32, 16, 128, 64, 8),
    (64, 8, 64, 16, 0),
    (512, 16, 128, 16, 8),
    (256, 128, 128, 64, 0),
    (8192, 2, 64, 16, 8),
]


def _prove_trace(z, case, ctx):
    n, blowup, bits, q, g = case
    return z.agg_prove_trace(random_trace_bytes(0xA66000 + n * 257 + blowup, n), PI_ELEMENTS, 5, 3, queries=q,
                             blowup=blowup, grind=g, min_security_bits=bits, check_air=False, ctx=ctx)


@pytest.mark.parametrize("case", TRACE_CASES, ids=lambda c: "n%d-b%d-%s-q%d-g%d" % (c[0], c[1], "fe2" if c[2] >= 128 else "fe", c[3], c[4]))
def test_device_equals_host_on_random_traces(z, gpu_ctx, case):
    want = _prove_trace(z, case, None)
    assert _prove_trace(z, case, gpu_ctx) == want


@pytest.fixture(scope="module")
def chain33(oracle, z):
    return chain_steps(oracle, z, 33, program=PROGRAM + 0x700, queries=4, grind=0)


def _real_entry(z, gpu_ctx, steps, **kw):
    want = z.agg_prove(steps, **kw)
    with z.agg_device_prover(1):
        got = z.agg_prove(steps, ctx=gpu_ctx, **kw)
    assert got == want
    z.agg_verify(got[0], kw.get("min_security_bits", 128))
    t = z.agg_last_times()
    assert len(t) == 6 and all(x >= 0 for x in t)
    with z.agg_device_prover(0):
        assert z.agg_prove(steps, ctx=gpu_ctx, **kw) == want


@pytest.mark.parametrize("case", sorted(AGG_CASES))
def test_real_entry_device_equals_host(oracle, z, gpu_ctx, case):
    _real_entry(z, gpu_ctx, chain_steps(oracle, z, **AGG_CASES[case]), grind=8)


@pytest.mark.parametrize("bits", [128, 64])
def test_real_entry_33_children(z, gpu_ctx, chain33, bits):
    """33 children: a 64-row trace, at the default options and in the base field."""
    assert len(z.agg_trace(chain33)[0]) == 64
    _real_entry(z, gpu_ctx, chain33, min_security_bits=bits)


def test_real_entry_reference_trace_mode(oracle, z, gpu_ctx):
    """partitions = 2 children: a non-zero root-error column, proved without the AIR pre-check."""
    steps = chain_steps(oracle, z, 3, program=PROGRAM + 0x603, queries=4, grind=0, partitions=2)
    want = z.agg_prove(steps, grind=8, trace_mode=z.AGG_TRACE_REFERENCE)
    assert want[0] != z.agg_prove(steps, grind=8)[0]
    assert z.agg_prove(steps, grind=8, trace_mode=z.AGG_TRACE_REFERENCE, ctx=gpu_ctx) == want
    with z.agg_device_prover(0):
        assert z.agg_prove(steps, grind=8, trace_mode=z.AGG_TRACE_REFERENCE, ctx=gpu_ctx) == want


def _message(z, fn):
    with pytest.raises(z.ZklError) as e:
        fn()
    return str(e.value)


def test_rejections_are_the_hosts(oracle, z, gpu_ctx):
    """The AIR pre-check runs on the host in front of either backend: a broken chain is rejected
    with the host path's message and the prover launches nothing."""
    broken = chain_steps(oracle, z, 2, program=PROGRAM + 0x300, break_chain_at=1)
    want = _message(z, lambda: z.agg_prove(broken, grind=8))
    assert "does not satisfy ZlAggAir" in want
    assert _message(z, lambda: z.agg_prove(broken, grind=8, ctx=gpu_ctx)) == want
    bad = random_trace_bytes(1, 8)
    want = _message(z, lambda: z.agg_prove_trace(bad, PI_ELEMENTS, 5, 3, queries=16, blowup=8, grind=0))
    assert "transition constraint" in want
    assert _message(z, lambda: z.agg_prove_trace(bad, PI_ELEMENTS, 5, 3, queries=16, blowup=8, grind=0,
                                                 ctx=gpu_ctx)) == want
    want = _message(z, lambda: z.agg_prove_trace(bad, PI_ELEMENTS, 5, 3, blowup=256, check_air=False))
    assert _message(z, lambda: z.agg_prove_trace(bad, PI_ELEMENTS, 5, 3, blowup=256, check_air=False,
                                                 ctx=gpu_ctx)) == want


def test_back_to_back_on_one_context(z, gpu_ctx):
    """Cached buffers reused at a smaller size after a larger one, then a segment proof between
    two aggregation proofs on the same context: each equals its host result."""
    big, small = (64, 16, 128, 16, 0), (8, 4, 128, 16, 0)
    want_big, want_small = _prove_trace(z, big, None), _prove_trace(z, small, None)
    before = z.pinned_bytes()[0]
    assert _prove_trace(z, big, gpu_ctx) == want_big
    held = z.pinned_bytes()[0]
    assert held >= before and held > 0
    assert _prove_trace(z, small, gpu_ctx) == want_small
    assert z.pinned_bytes()[0] == held  # the staging of the larger call served the smaller one
    n = 1 << 5
    t, pi, w = z.synth_vm_segment(0x5EED0A66, 5)
    opts = z.proof_options(w, n, queries=8, blowup=16, grind=0)
    seg = gpu_ctx.prove_segment(t, w, n, pi, opts)
    assert _prove_trace(z, big, gpu_ctx) == want_big
    assert gpu_ctx.prove_segment(t, w, n, pi, opts) == seg
    z.verify_segment(seg, pi, opts)
