"""One rank of tests/test_gpu_agg_session.py::test_feed_rounds_through_the_stub (test
infrastructure): dist.feed_rounds over zkl_comm_gather_bytes through the NCCL-ABI shared-memory
stub (ZKL_RCCL_LIB), two processes on one GPU.

    python tests/agg_rounds_stub_worker.py <rank> <world> <uid hex>

Every rank makes the same five chained children and hands over its share in two rounds (sizes
(2, 1) and (1, 1)); rank 0 feeds a session on its context and compares the artifact with the
host's agg_prove.  Prints one JSON line; exit 0 / 5 (wrong bytes)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zk-lisp_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    rank, world, uid = int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3])
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import oracle_lib
    import zkl_hip
    from test_agg_session import ROUNDS, ROUNDS_PROGRAM
    from test_batch_verify import chain_steps
    from zkl_hip import dist
    oracle_lib.build()
    steps = chain_steps(oracle_lib, zkl_hip, 5, program=ROUNDS_PROGRAM, queries=4, grind=0)
    rounds = [[(i, steps[i]) for i in r] for r in ROUNDS[rank]]
    comm = zkl_hip.Comm(0, world, rank, uid)
    res = {"rank": rank, "added": None, "equal": None}
    try:
        if rank == 0:
            ctx = zkl_hip.Context(0)
            try:
                with zkl_hip.AggSession(5, ctx=ctx, grind=8) as s:
                    res["added"] = dist.feed_rounds(rounds, s, comm)
                    res["equal"] = s.finish() == zkl_hip.agg_prove(steps, grind=8)
            finally:
                ctx.close()
        else:
            res["added"] = dist.feed_rounds(rounds, None, comm)
    finally:
        comm.close()
    print(json.dumps(res), flush=True)
    return 0 if rank != 0 or res["equal"] else 5


if __name__ == "__main__":
    sys.exit(main())
