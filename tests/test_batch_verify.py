"""Batch verification on the host (zkl_hip_verify_segments with ctx NULL): a
batch of segment proofs gets, entry for entry, the verdict and message zkl_verify_segment
gives each proof alone, and the aggregation prover run through the same plan / executor split
returns the bytes it returned before.  The device path is checked in
tests/test_gpu_batch_verify.py; the helpers here are shared with it."""
import ctypes as C
import random

import pytest

CASES = [  # tests/test_verifier.py CASES: seed, log_n, flags, q, blowup, grind, partitions
    (0x5EED0B01, 5, 0, 8, 16, 2, 1),
    (0x5EED0B02, 6, 0, 32, 8, 4, 1),
    (0x5EED0B03, 7, 1, 24, 8, 3, 1),
    (0x5EED0B04, 8, 2, 16, 16, 2, 2),
    (0x5EED0B05, 8, 4, 16, 16, 0, 1),
    (0x5EED0B06, 8, 7, 12, 32, 1, 4),
    (0x5EED0B07, 6, 0, 255, 8, 1, 1),
    (0x5EED0B08, 9, 6, 40, 16, 5, 1),
]


def lib_pi(zkl_hip, opi):
    pi = zkl_hip.AirPublicInputs()
    C.memmove(C.byref(pi), C.byref(opi), C.sizeof(pi))
    return pi


def lib_opts(zkl_hip, oo):
    return zkl_hip.ProofOptions(*[getattr(oo, f) for f, _ in oo._fields_])


def oracle_proof(oracle, zkl_hip, seed, log_n, flags, q, blowup, grind, parts):
    n = 1 << log_n
    t, opi, w = oracle.synth_segment(seed, log_n, flags)
    oo = oracle.default_options(w, n, queries=q, blowup=blowup, grind=grind)
    oo.num_partitions = parts
    return oracle.prove(t, w, n, opi, oo), lib_pi(zkl_hip, opi), lib_opts(zkl_hip, oo)


def accept_batch(oracle, zkl_hip):
    """The eight CASES of tests/test_verifier.py as (proofs, pis, opts)."""
    b = [oracle_proof(oracle, zkl_hip, *c) for c in CASES]
    return [x[0] for x in b], [x[1] for x in b], [x[2] for x in b]


def corruption_batch(oracle, zkl_hip):
    """The 200 single-byte corruptions of test_library_verifier_rejects_corruptions_like_the_oracle
    (same seed and generator), with the untouched proof at the first, middle and last index."""
    proof, pi, o = oracle_proof(oracle, zkl_hip, 0x5EED0B10, 6, 0, 16, 8, 2, 1)
    rng = random.Random(3)
    proofs = []
    for k in range(200):
        b = bytearray(proof)
        i = rng.randrange(len(b)) if k % 4 else (k * 7919) % len(b)
        b[i] ^= 1 << rng.randrange(8)
        proofs.append(bytes(b))
    proofs = [proof] + proofs[:100] + [proof] + proofs[100:] + [proof]
    return proofs, [pi] * len(proofs), [o] * len(proofs)


PROGRAM = 0x5EEDA900


def chain_steps(oracle, zkl_hip, count, log_n=5, flags=0, program=PROGRAM, break_chain_at=None, queries=8, grind=4,
                partitions=None):
    """tests/test_agg.py::_steps: count chained segments -> oracle proofs -> zl1 steps."""
    n = 1 << log_n
    rom0, out = 0, []
    for i in range(count):
        t, pi, w = oracle.synth_segment_chain(program, program + i, log_n, rom0 if i != break_chain_at else rom0 + 1,
                                              flags)
        opts = oracle.default_options(w, n, queries=queries, grind=grind)
        if partitions:
            opts.num_partitions = partitions
        proof = oracle.prove(t, w, n, pi, opts)
        zpi = lib_pi(zkl_hip, pi)
        info = zkl_hip.step_info_for(zpi, i, count, i.to_bytes(32, "little"), (i + 1).to_bytes(32, "little"))
        out.append(zkl_hip.step_proof_encode(zpi, info, proof))
        rom0 = pi.rom_s_out[0].lo | (pi.rom_s_out[0].hi << 64)
    return out


def single_message(zkl_hip, proof, pi, o):
    """What verify_segment says about one proof: "" or the failing check."""
    try:
        zkl_hip.verify_segment(proof, pi, o)
        return ""
    except zkl_hip.ZklError as e:
        head = str(zkl_hip.ZklError(e.code, ""))
        assert str(e).startswith(head)
        return str(e)[len(head):]


def test_batch_accepts_the_verifier_cases(oracle):
    import zkl_hip
    proofs, pis, opts = accept_batch(oracle, zkl_hip)
    assert zkl_hip.verify_segments(proofs, pis, opts) == [""] * 8
    assert zkl_hip.verify_segments([], [], []) == []


def test_batch_messages_equal_single_proof_messages(oracle):
    import zkl_hip
    proofs, pis, opts = corruption_batch(oracle, zkl_hip)
    want = [single_message(zkl_hip, p, pi, o) for p, pi, o in zip(proofs, pis, opts)]
    got = zkl_hip.verify_segments(proofs, pis, opts)
    assert len(got) == 203
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"entry {k}"
    assert got[0] == got[101] == got[202] == ""
    assert sum(1 for m in got if m) >= 190
    assert len(set(got)) > 5  # the corruptions hit many different checks


def test_aggregation_with_null_context_is_agg_prove(oracle):
    import zkl_hip
    steps = chain_steps(oracle, zkl_hip, 3)
    want = zkl_hip.agg_prove(steps, grind=8)
    assert zkl_hip.agg_prove(steps, grind=8, ctx=None) == want
    t = zkl_hip.agg_last_times()
    assert len(t) == 6 and all(x >= 0 for x in t)
    assert t[5] >= t[0]
    assert t[5] > 0
