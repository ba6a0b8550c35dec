"""Aggregation session on the host (zkl_hip_agg_begin / _add / _finish with ctx NULL, DESIGN.md
§10): step proofs added one at a time, in any order and from several threads, give the artifact,
the digest and the rejections of the one-shot zkl_agg_prove, which is itself begin, adds, finish
over the same code.  The device path is checked in tests/test_gpu_agg_session.py; the helpers
here are shared with it.  Children are tests/test_agg.py::_steps: oracle proofs of 32-row
segments of one synthetic chain."""
import hashlib
import os
import random
import socket
import sys
import threading

import pytest

from test_agg import PROGRAM, _steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import agg_ref  # noqa: E402

ORDERS = ("in_order", "reversed", "shuffled", "threads")
# feed_rounds at world size 2: per rank, the segment indices of each round (sizes (2, 1) and (1, 1))
ROUNDS = {0: [[0, 1], [3]], 1: [[2], [4]]}
ROUNDS_PROGRAM = PROGRAM + 0xA05


@pytest.fixture(scope="module")
def z():
    import zkl_hip
    return zkl_hip


_chains = {}


def chain(oracle, z, n):
    """n chained children (queries 4, grind 0), made once per count."""
    if n not in _chains:
        _chains[n] = _steps(oracle, z, n, program=PROGRAM + 0xA00 + n, queries=4, grind=0)
    return _chains[n]


def session_prove(z, steps, order, ctx=None, **kw):
    """(artifact, digest) of a session over `steps` with the adds in `order`."""
    n = len(steps)
    with z.AggSession(n, ctx=ctx, **kw) as s:
        if order == "threads":
            errors = []

            def work(k):
                try:
                    for p in range(k, n, 4):
                        s.add(p, steps[p])
                except Exception as e:  # noqa: BLE001
                    errors.append(e)
            th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not errors, errors
        else:
            pos = list(range(n))
            if order == "reversed":
                pos.reverse()
            elif order == "shuffled":
                random.Random(0xA66 + n).shuffle(pos)
            for p in pos:
                s.add(p, steps[p])
        out = s.finish()
        t = s.times()
        assert len(t) == 6 and all(x >= 0 for x in t) and t[5] > 0 and t[0] > 0
    return out


def message(z, fn):
    with pytest.raises(z.ZklError) as e:
        fn()
    return str(e.value)


@pytest.mark.parametrize("bits", [128, 64])
@pytest.mark.parametrize("n", [1, 3, 8, 9])
def test_session_equals_one_shot(oracle, z, n, bits):
    """n = 8: a power of two, the valid mode's padding row doubles the trace; n = 9 does not."""
    steps = chain(oracle, z, n)
    want = z.agg_prove(steps, grind=8, min_security_bits=bits)
    assert len(z.agg_trace(steps)[0]) == (8 if n < 8 else 16)
    for order in ORDERS:
        assert session_prove(z, steps, order, grind=8, min_security_bits=bits) == want, order


@pytest.mark.parametrize("count", [3, 8])
def test_session_reference_trace_mode(oracle, z, count):
    """The inputs of test_reference_trace_mode_matches_restatement: children proved with two
    partitions, whose constraint root errors are non-zero in the reference mode."""
    steps = _steps(oracle, z, count, program=PROGRAM + 0x600 + count, queries=4, grind=0, partitions=2)
    want = z.agg_prove(steps, grind=8, trace_mode=z.AGG_TRACE_REFERENCE)
    assert want != z.agg_prove(steps, grind=8)
    for order in ("reversed", "threads"):
        assert session_prove(z, steps, order, grind=8, trace_mode=z.AGG_TRACE_REFERENCE) == want


def test_one_shot_still_gives_the_stable_artifact(oracle, z):
    """zkl_agg_prove, now a session inside, on the inputs of test_artifact_hash_is_stable (chain3,
    grind 12): the artifact of the independent restatement oracle/agg_ref.py, twice."""
    chain3 = _steps(oracle, z, 3)
    want, want_dg, _ = agg_ref.agg_prove(oracle, chain3, grind=12)
    a1, d1 = z.agg_prove(chain3, grind=12)
    a2, _ = z.agg_prove(chain3, grind=12)
    assert hashlib.sha256(a1).digest() == hashlib.sha256(a2).digest() == hashlib.sha256(want).digest()
    assert d1 == want_dg
    assert session_prove(z, chain3, "shuffled", grind=12) == (want, want_dg)


def _corrupt(step):
    bad = bytearray(step)
    bad[-200] ^= 1
    return bytes(bad)


def test_corrupted_child_is_refused_at_add(oracle, z):
    st = list(chain(oracle, z, 3))
    st[1] = _corrupt(st[1])
    want = message(z, lambda: z.agg_prove(st, grind=8))
    assert "child 1: child step proof does not replay" in want
    with z.AggSession(3, grind=8) as s:
        s.add(2, st[2])
        assert message(z, lambda: s.add(1, st[1])) == want
        s.add(0, st[0])  # a refused child does not stop later adds
        assert message(z, s.finish) == want


@pytest.mark.parametrize("first", [4, 1])
def test_two_corrupted_children_finish_names_the_lower(oracle, z, first):
    st = list(chain(oracle, z, 9))
    st[1], st[4] = _corrupt(st[1]), _corrupt(st[4])
    want = message(z, lambda: z.agg_prove(st, grind=8))
    assert want.split(":")[1].strip() == "child 1"
    with z.AggSession(9, grind=8) as s:
        for p in [first, 5 - first] + [p for p in range(9) if p not in (1, 4)]:
            if p in (1, 4):
                assert ("child %d:" % p) in message(z, lambda: s.add(p, st[p]))
            else:
                s.add(p, st[p])
        assert message(z, s.finish) == want


def test_cross_child_rejections_come_at_finish(oracle, z):
    # ROM lane 0 not carried from segment 0 to 1
    broken = _steps(oracle, z, 2, program=PROGRAM + 0x300, break_chain_at=1)
    want = message(z, lambda: z.agg_prove(broken, grind=8))
    assert "does not satisfy ZlAggAir" in want
    with z.AggSession(2, grind=8) as s:
        s.add(1, broken[1])
        s.add(0, broken[0])
        assert message(z, s.finish) == want
    # a child of another program
    mixed = [chain(oracle, z, 3)[0], _steps(oracle, z, 1, program=PROGRAM + 0x400)[0]]
    want = message(z, lambda: z.agg_prove(mixed, grind=8))
    with z.AggSession(2, grind=8) as s:
        s.add(0, mixed[0])
        s.add(1, mixed[1])
        assert message(z, s.finish) == want


def test_session_misuse_is_refused(oracle, z):
    st = chain(oracle, z, 3)
    want = z.agg_prove(st, grind=8)
    with z.AggSession(3, grind=8) as s:
        s.add(0, st[0])
        assert "already added" in message(z, lambda: s.add(0, st[0]))
        assert "out of range" in message(z, lambda: s.add(3, st[0]))
        s.add(2, st[2])
        s.add(1, st[1])
        assert s.finish() == want  # the refused adds changed nothing
        assert "finish was already called" in message(z, s.finish)
    with z.AggSession(3, grind=8) as s:
        s.add(0, st[0])
        s.add(2, st[2])
        assert "2 of 3 step proofs added" in message(z, s.finish)
        assert "finish was already called" in message(z, s.finish)
    s = z.AggSession(3, grind=8)  # free without finish
    s.add(1, st[1])
    s.close()
    s.close()
    with pytest.raises(z.ZklError, match="closed"):
        s.add(0, st[0])


@pytest.mark.parametrize("kw", [dict(queries=256), dict(grind=33), dict(grind=8, trace_mode=2),
                                dict(queries=16, blowup=8, grind=0)], ids=["queries", "grind", "mode", "security"])
def test_begin_checks_the_options(oracle, z, kw):
    """begin refuses what the one-shot call refuses, with its text, before any child is seen."""
    want = message(z, lambda: z.agg_prove(chain(oracle, z, 3), **kw))
    assert message(z, lambda: z.AggSession(3, **kw)) == want


def test_begin_refuses_an_empty_batch(z):
    assert message(z, lambda: z.AggSession(0)) == message(z, lambda: z.agg_prove([]))


# ---- dist.feed_rounds at world size 2 over gloo -----------------------------------------------
def _rounds_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    for p in (os.path.join(ROOT, "zk-lisp_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import oracle_lib
    import zkl_hip
    from zkl_hip import dist
    oracle_lib.build()
    dist.init()
    steps = _steps(oracle_lib, zkl_hip, 5, program=ROUNDS_PROGRAM, queries=4, grind=0)
    rounds = [[(i, steps[i]) for i in r] for r in ROUNDS[rank]]
    if rank == 0:
        with zkl_hip.AggSession(5, grind=8) as s:
            added = dist.feed_rounds(rounds, s)
            q.put((rank, added, s.finish()))
    else:
        q.put((rank, dist.feed_rounds(rounds, None), None))
    dist.shutdown()


def test_feed_rounds_world_size_2(oracle, z):
    """5 children in two rounds of sizes (2, 1) and (1, 1): rank 0's session, fed from its worker
    thread as the rounds arrive, gives agg_prove's artifact."""
    # the ranks import torch themselves; starting them needs only the standard library
    import multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rounds_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r, added, out = q.get(timeout=180)
        res[r] = (added, out)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[1] == (None, None)
    steps = _steps(oracle, z, 5, program=ROUNDS_PROGRAM, queries=4, grind=0)
    assert res[0] == (5, z.agg_prove(steps, grind=8))
