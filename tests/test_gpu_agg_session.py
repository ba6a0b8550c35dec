"""Aggregation session on the device (zkl_hip_agg_begin / _add / _finish with a context), the
aggregation proof's grinding on the context's stream, prove_chain and the hand-off in rounds
(DESIGN.md §10): every artifact and digest equals what the one-shot calls and the host search
give.  Children are oracle proofs of 32-row segments, as in tests/test_agg_session.py."""
import json
import os
import subprocess
import sys
import threading

import pytest

from test_agg_session import ORDERS, ROOT, chain, session_prove
from test_batch_verify import PROGRAM, chain_steps
from test_comm_stub import STUB, _env, _py

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "agg_rounds_stub_worker.py")


@pytest.fixture(scope="module")
def z():
    import zkl_hip
    return zkl_hip


@pytest.mark.parametrize("bits", [128, 64])
@pytest.mark.parametrize("n", [3, 9])
def test_device_session_equals_one_shot(oracle, z, gpu_ctx, n, bits):
    steps = chain(oracle, z, n)
    want = z.agg_prove(steps, grind=8, min_security_bits=bits)
    assert z.agg_prove(steps, grind=8, min_security_bits=bits, ctx=gpu_ctx) == want
    for order in ORDERS:
        assert session_prove(z, steps, order, ctx=gpu_ctx, grind=8, min_security_bits=bits) == want, order


def test_device_session_33_children_shuffled(oracle, z, gpu_ctx):
    """The 33-child chain of tests/test_gpu_agg_prover.py (a 64-row trace), at the default options."""
    steps = chain_steps(oracle, z, 33, program=PROGRAM + 0x700, queries=4, grind=0)
    want = z.agg_prove(steps, ctx=gpu_ctx)
    assert session_prove(z, steps, "shuffled", ctx=gpu_ctx) == want
    z.agg_verify(want[0])


def test_device_session_refuses_a_corrupted_child_like_the_host(oracle, z, gpu_ctx):
    st = list(chain(oracle, z, 3))
    bad = bytearray(st[1])
    bad[-200] ^= 1
    st[1] = bytes(bad)
    with pytest.raises(z.ZklError) as e:
        z.agg_prove(st, grind=8)
    with z.AggSession(3, ctx=gpu_ctx, grind=8) as s:
        s.add(0, st[0])
        with pytest.raises(z.ZklError) as got:
            s.add(1, st[1])
        assert str(got.value) == str(e.value)
        s.add(2, st[2])
        with pytest.raises(z.ZklError) as got:
            s.finish()
        assert str(got.value) == str(e.value)


# ---- the aggregation proof's grinding on the device ---------------------------------------------
@pytest.mark.parametrize("grind", [0, 4, 8, 16])
def test_device_grinding_finds_the_host_nonce(oracle, z, gpu_ctx, grind):
    steps = chain(oracle, z, 3)
    want = z.agg_prove(steps, grind=grind)
    with z.agg_device_prover(1):
        assert z.agg_prove(steps, grind=grind, ctx=gpu_ctx) == want
        t = z.agg_last_times()
        assert len(t) == 6 and t[4] >= 0
    with z.agg_device_prover(0):  # the search on host threads
        assert z.agg_prove(steps, grind=grind, ctx=gpu_ctx) == want


def test_device_grinding_over_several_windows(oracle, z, gpu_ctx, monkeypatch):
    """Grind 20 on the 9-child chain: windows of 2^20 tries, so with probability 1 / e the first
    one is empty.  Then the same with the first window shrunk to 16 tries (the segment prover's test
    hook) at grind 8: the expected 256 tries take several windows and several read-backs."""
    steps = chain(oracle, z, 9)
    want = z.agg_prove(steps, grind=20)
    with z.agg_device_prover(1):
        assert z.agg_prove(steps, grind=20, ctx=gpu_ctx) == want
        want8 = z.agg_prove(steps, grind=8)
        monkeypatch.setenv("ZKL_TEST_GRIND_FIRST", "16")
        assert z.agg_prove(steps, grind=8, ctx=gpu_ctx) == want8
        assert z.agg_prove(steps, grind=8, min_security_bits=64, ctx=gpu_ctx) == \
            z.agg_prove(steps, grind=8, min_security_bits=64)


# ---- prove_chain ----------------------------------------------------------------------------------
@pytest.mark.parametrize("device_build", [False, True])
def test_prove_chain_on_multiseg(z, gpu_ctx, device_build):
    from test_segments import PID, multiseg_ops
    from zkl_hip.program import prove_chain, prove_program, steps_of
    ops = multiseg_ops()
    P = z.Program(ops, PID)
    plan = z.plan_segments(len(ops), 1 << 10)
    assert len(plan) == 2
    kw = dict(inflight=2, builders=2, queries=8, grind=4, device_build=device_build)
    agg = dict(queries=64, blowup=16, grind=8)
    got = prove_chain(P, plan, agg_queries=64, agg_blowup=16, agg_grind=8, **kw)
    steps = steps_of(prove_program(P, plan, **kw).values(), len(plan))
    assert got["steps"] == steps
    assert (got["artifact"], got["digest"]) == z.agg_prove(steps, ctx=gpu_ctx, **agg)
    z.agg_verify(got["artifact"])
    assert got["tail_ms"] > 0 and len(got["times"]) == 6 and all(x >= 0 for x in got["times"])
    # the session on a context the caller passes
    again = prove_chain(P, plan, agg_ctx=gpu_ctx, agg_queries=64, agg_blowup=16, agg_grind=8, **kw)
    assert again["artifact"] == got["artifact"]
    P.close()


# ---- concurrency ----------------------------------------------------------------------------------
def test_two_sessions_on_two_contexts(oracle, z, gpu_ctx):
    chains = {0: chain(oracle, z, 9), 1: chain(oracle, z, 3)}
    want = {k: z.agg_prove(v, grind=8) for k, v in chains.items()}
    other = z.Context(0)
    got, errors = {}, []

    def work(k, ctx):
        try:
            got[k] = session_prove(z, chains[k], "threads", ctx=ctx, grind=8)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    try:
        one_after_the_other = {0: session_prove(z, chains[0], "in_order", ctx=gpu_ctx, grind=8),
                               1: session_prove(z, chains[1], "in_order", ctx=other, grind=8)}
        th = [threading.Thread(target=work, args=(0, gpu_ctx)), threading.Thread(target=work, args=(1, other))]
        for x in th:
            x.start()
        for x in th:
            x.join()
    finally:
        other.close()
    assert not errors, errors
    assert got == one_after_the_other == want


# ---- dist.feed_rounds through the NCCL-ABI stub: two processes on one GPU -------------------------
@pytest.mark.timeout(300)
def test_feed_rounds_through_the_stub(oracle, z):
    assert os.path.exists(STUB)
    r = _py("import zkl_hip; print(zkl_hip.comm_unique_id().hex())")
    assert r.returncode == 0, r.stderr
    uid = r.stdout.strip()
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, WORKER, str(k), "2", uid], env=_env(),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k in range(2)]
    out = []
    for p in procs:
        so, se = p.communicate(timeout=240)
        out.append((p.returncode, so, se))
    for rc, so, se in out:
        assert rc == 0, (rc, so, se[-2000:])
    lines = {ln["rank"]: ln for ln in (json.loads(so.strip().splitlines()[-1]) for _, so, _ in out)}
    assert lines[1]["added"] is None
    assert lines[0]["added"] == 5 and lines[0]["equal"] is True
