"""Stage entry point of the aggregation prover (zkl_hip_agg_prove_trace, host backend, no GPU):
the ZlAggAir proof of a caller's trace against oracle/agg_ref.py's prove_agg and against the
proof inside agg_prove's artifact, its rejections, and the device-prover switch."""
import os
import random
import subprocess
import sys

import pytest

from test_batch_verify import PROGRAM, chain_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import agg_ref  # noqa: E402

ZKL_E_INVALID = -1


@pytest.fixture(scope="module")
def z():
    import zkl_hip
    return zkl_hip


def public_of(oracle, steps):
    return agg_ref.build_public(oracle, [agg_ref.decode_step(oracle, s) for s in steps])


def random_trace(seed, n):
    """31 columns of n canonical field elements (the top byte cleared: below the modulus)."""
    rng = random.Random(seed)
    return [[rng.getrandbits(120) for _ in range(n)] for _ in range(31)]


@pytest.fixture(scope="module")
def one_child_public(oracle, z):
    return public_of(oracle, chain_steps(oracle, z, 1, program=PROGRAM + 0x100))


@pytest.fixture(scope="module")
def chain3(oracle, z):
    return chain_steps(oracle, z, 3)


def _invalid(z, fn):
    with pytest.raises(z.ZklError) as e:
        fn()
    assert e.value.code == ZKL_E_INVALID
    return str(e.value)


@pytest.mark.parametrize("n,blowup,ext", [(8, 2, 2), (8, 16, 1), (16, 8, 2)])
def test_stage_entry_matches_restatement(oracle, z, one_child_public, n, blowup, ext):
    p = one_child_public
    T = random_trace(0xA66 + n * 131 + blowup, n)
    want = agg_ref.prove_agg(oracle, T, p, 16, blowup, 4, ext, check_air=False)
    got = z.agg_prove_trace(T, agg_ref.agg_pi_elements(p), p["v_units_total"], p["children_count"], queries=16,
                            blowup=blowup, grind=4, min_security_bits=128 if ext == 2 else 64, check_air=False)
    assert got == bytes(want)


@pytest.mark.parametrize("bits", [128, 64])
def test_stage_entry_gives_the_artifacts_proof(oracle, z, chain3, bits):
    art, _ = z.agg_prove(chain3, grind=8, min_security_bits=bits)
    p = public_of(oracle, chain3)
    T = z.agg_trace(chain3)
    got = z.agg_prove_trace(T, agg_ref.agg_pi_elements(p), p["v_units_total"], p["children_count"], grind=8,
                            min_security_bits=bits, check_air=True)
    assert got == z.parse_agg_artifact(art)["proof"]
    assert art.endswith(got)
    # the column-major bytes are the same trace
    raw = b"".join(v.to_bytes(16, "little") for c in T for v in c)
    assert z.agg_prove_trace(raw, agg_ref.agg_pi_elements(p), p["v_units_total"], p["children_count"], grind=8,
                             min_security_bits=bits) == got


def test_rejections_without_a_device(oracle, z, chain3):
    p = public_of(oracle, chain3)
    el = agg_ref.agg_pi_elements(p)
    T = z.agg_trace(chain3)

    def go(trace=T, **kw):
        args = dict(queries=16, blowup=8, grind=4, check_air=False)
        args.update(kw)
        return z.agg_prove_trace(trace, el, p["v_units_total"], p["children_count"], **args)

    assert go(check_air=True)  # the arguments below are what is rejected, not these
    for rows in (12, 4, 1 << 14):
        assert "rows" in _invalid(z, lambda: go(trace=bytes(31 * 16 * rows)))
    for blowup in (1, 256, 12):
        assert "blowup" in _invalid(z, lambda: go(blowup=blowup))
    assert "queries" in _invalid(z, lambda: go(queries=256))
    assert "grinding" in _invalid(z, lambda: go(grind=33))
    assert "canonical" in _invalid(z, lambda: go(trace=b"\xff" * (31 * 16 * 8)))
    # a trace violating C11 (the child counter skips a step): the host path's message
    bad = [list(c) for c in T]
    bad[agg_ref.CNT][2] += 1
    msg = _invalid(z, lambda: go(trace=bad, check_air=True))
    assert "aggregation trace does not satisfy ZlAggAir: transition constraint C11 fails at row 1" in msg
    assert go(trace=bad)  # check_air off proves it anyway
    # the same violation through agg_prove keeps its message
    broken = chain_steps(oracle, z, 2, program=PROGRAM + 0x300, break_chain_at=1)
    assert "does not satisfy ZlAggAir" in _invalid(z, lambda: z.agg_prove(broken, grind=8))
    # an assertion: the public total differs from the last row's accumulator
    msg = _invalid(z, lambda: z.agg_prove_trace(T, el, p["v_units_total"] + 1, p["children_count"], queries=16,
                                                blowup=8, grind=4))
    assert msg.endswith("aggregation trace does not satisfy ZlAggAir: an assertion fails")


def test_device_prover_switch(z):
    lib = z.load_library()
    assert lib.zkl_hip_agg_device_prover() == 1
    with z.agg_device_prover(0):
        assert lib.zkl_hip_agg_device_prover() == 0
        with z.agg_device_prover(True):
            assert lib.zkl_hip_agg_device_prover() == 1
        assert lib.zkl_hip_agg_device_prover() == 0
    assert lib.zkl_hip_agg_device_prover() == 1
    assert lib.zkl_hip_set_agg_device_prover(2) == ZKL_E_INVALID
    assert lib.zkl_hip_agg_device_prover() == 1


@pytest.mark.parametrize("env,want", [("0", 0), ("1", 1), (None, 1)])
def test_device_prover_switch_reads_the_environment(env, want):
    e = {k: v for k, v in os.environ.items() if k != "ZKL_AGG_DEVICE_PROVER"}
    if env is not None:
        e["ZKL_AGG_DEVICE_PROVER"] = env
    code = ("import sys; sys.path.insert(0, %r); import zkl_hip; "
            "print(zkl_hip.load_library().zkl_hip_agg_device_prover())" % os.path.join(ROOT, "zk-lisp_amd"))
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == str(want)
