"""Batch verification on the device (zkl_hip_verify_segments / zkl_hip_agg_prove with a context,
DESIGN.md §10): the Poseidon hashing of the openings and the coefficient draws run in
open_rows_kernel / merge_jobs_kernel / launch_draws, and every verdict, message, artifact and
digest equals the host path's.  Inputs are oracle proofs of tiny synthetic segments; the only
thing ever corrupted is proof bytes handed to the verifier."""
import itertools

import pytest

from test_batch_verify import (CASES, PROGRAM, accept_batch, chain_steps, corruption_batch, oracle_proof,
                               single_message)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    import zkl_hip
    return zkl_hip


@pytest.fixture(scope="module")
def accept(oracle, z):
    return accept_batch(oracle, z)


def _host_messages(z, batch):
    return [single_message(z, p, pi, o) for p, pi, o in zip(*batch)]


def test_device_accepts_the_verifier_cases(z, accept, gpu_ctx):
    assert z.verify_segments(*accept, ctx=gpu_ctx) == [""] * len(CASES)


@pytest.mark.parametrize("rule", [0, 1])
def test_one_chunk_rows_under_both_row_digest_rules(z, accept, gpu_ctx, rule):
    """The partitions-2 case (composition rows of one chunk): under rule 0 it verifies and, in the
    aggregation, schedules the rule-1 re-hash; under rule 1 the host rejects the constraint
    opening, and so must the device, with the same words."""
    k = [c[6] for c in CASES].index(2)
    one = tuple([x[k]] for x in accept)
    with z.row_digest_rule(rule):
        want = _host_messages(z, one)
        got = z.verify_segments(*one, ctx=gpu_ctx)
    assert got == want
    assert (got == [""]) == (rule == 0)
    if rule:
        assert "constraint Merkle opening" in got[0]


def test_device_messages_equal_host_messages_on_corruptions(oracle, z, gpu_ctx):
    """203 proofs, 200 of them with one flipped byte.  A flipped root or nonce changes the drawn
    positions: the plan builder rejects the opening on the host with the host verifier's message
    and the proof contributes no tree to the device."""
    batch = corruption_batch(oracle, z)
    want = _host_messages(z, batch)
    got = z.verify_segments(*batch, ctx=gpu_ctx)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"entry {k}"
    assert got[0] == got[101] == got[202] == "" and sum(1 for m in got if m) >= 190


def _unique_queries(proof):
    return proof[6 + 1 + 16 + 10]  # num_unique_queries, after TraceInfo, the modulus and ProofOptions


def test_launch_size_edges(oracle, z, gpu_ctx):
    """One block holds 20 groups.  (a) one proof with one query: one job in every launch.
    (b) proofs of one row shape whose opened trace rows number 20 k + 1: a last block with one
    live group."""
    p1 = oracle_proof(oracle, z, 0x5EED0C01, 5, 0, 1, 8, 0, 1)
    assert _unique_queries(p1[0]) == 1
    assert z.verify_segments([p1[0]], [p1[1]], [p1[2]], ctx=gpu_ctx) == [""]
    pool = [oracle_proof(oracle, z, 0x5EED0C10 + i, 5, 0, 7, 8, 0, 1) for i in range(4)]
    nq = [_unique_queries(p[0]) for p in pool]
    pick = next((c for r in range(1, 9) for c in itertools.combinations_with_replacement(range(4), r)
                 if sum(nq[i] for i in c) % 20 == 1 and sum(nq[i] for i in c) > 20), None)
    assert pick is not None, nq
    batch = [pool[i] for i in pick]
    # the counts are those of verified positions: each proof verifies on the host
    assert [single_message(z, *b) for b in batch] == [""] * len(batch)
    rows = sum(_unique_queries(b[0]) for b in batch)
    assert rows % 20 == 1 and rows > 20
    assert z.verify_segments([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch], ctx=gpu_ctx) == \
        [""] * len(batch)


AGG_CASES = {
    "one": dict(count=1, program=PROGRAM + 0x100),
    "three": dict(count=3),
    "eight": dict(count=8, program=PROGRAM + 0x500, queries=4, grind=0),
    "w212": dict(count=2, log_n=6, flags=2, program=PROGRAM + 0x202),
    "sponge": dict(count=2, log_n=6, flags=1, program=PROGRAM + 0x201),
}


@pytest.mark.parametrize("case", sorted(AGG_CASES))
def test_aggregation_parity(oracle, z, gpu_ctx, case):
    steps = chain_steps(oracle, z, **AGG_CASES[case])
    want = z.agg_prove(steps, grind=8)
    assert z.agg_prove(steps, grind=8, ctx=gpu_ctx) == want
    t = z.agg_last_times()
    assert len(t) == 6 and all(x >= 0 for x in t) and t[5] >= t[1] > 0


def test_aggregation_parity_reference_trace_mode(oracle, z, gpu_ctx):
    """partitions = 2: the composition rows are one chunk, the rule-1 roots differ from the
    committed ones and reach the artifact through the root-error column."""
    steps = chain_steps(oracle, z, 3, program=PROGRAM + 0x603, queries=4, grind=0, partitions=2)
    want = z.agg_prove(steps, grind=8, trace_mode=z.AGG_TRACE_REFERENCE)
    assert want[0] != z.agg_prove(steps, grind=8)[0]
    assert z.agg_prove(steps, grind=8, trace_mode=z.AGG_TRACE_REFERENCE, ctx=gpu_ctx) == want


def _vint(b, off):
    b0 = b[off]
    if b0 == 0:
        return int.from_bytes(b[off + 1:off + 9], "little"), off + 9
    ln = (b0 & -b0).bit_length()
    return int.from_bytes(b[off:off + ln], "little") >> ln, off + ln


def _flip_trace_query_value(z, step):
    """One bit of the first opened trace row of the step's inner proof."""
    inner = z.parse_step_proof(step)["inner"]
    base = len(step) - len(inner)
    assert step[base:] == inner
    clen, off = _vint(inner, 34)          # commitments
    one, off = _vint(inner, off + clen)   # number of trace segments
    assert one == 1
    tlen, off = _vint(inner, off)         # trace query values
    assert tlen > 16
    b = bytearray(step)
    b[base + off + 5] ^= 1
    return bytes(b)


def _message(z, fn):
    with pytest.raises(z.ZklError) as e:
        fn()
    return str(e.value)


def test_aggregation_rejections_match_the_host(oracle, z, gpu_ctx):
    steps = chain_steps(oracle, z, 3)
    bad = [steps[0], _flip_trace_query_value(z, steps[1]), steps[2]]
    want = _message(z, lambda: z.agg_prove(bad, grind=8))
    assert "child 1" in want and "trace Merkle opening" in want
    assert _message(z, lambda: z.agg_prove(bad, grind=8, ctx=gpu_ctx)) == want
    broken = chain_steps(oracle, z, 2, program=PROGRAM + 0x300, break_chain_at=1)
    want = _message(z, lambda: z.agg_prove(broken, grind=8))
    assert "does not satisfy ZlAggAir" in want
    assert _message(z, lambda: z.agg_prove(broken, grind=8, ctx=gpu_ctx)) == want


def test_staging_is_pinned_accounted_and_reused(z, accept, gpu_ctx):
    before, _ = z.pinned_bytes()
    assert z.verify_segments(*accept, ctx=gpu_ctx) == [""] * len(CASES)
    cur1, peak1 = z.pinned_bytes()
    assert before <= cur1 <= peak1 and cur1 > 0
    assert z.verify_segments(*accept, ctx=gpu_ctx) == [""] * len(CASES)
    cur2, peak2 = z.pinned_bytes()
    assert cur2 == cur1 and cur2 <= peak2
