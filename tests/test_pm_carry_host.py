"""The matrix-core Poseidon round's cube and fold on the host (zk-lisp_amd/csrc/mont26.h:
mont_cube130_chain, pm_normalise) through the stand-alone program tests/cpp/pm_carry_test: limb
equality with mont_cube130, canonical equality with the fold as it was before the 32-bit carries,
plain arithmetic mod p, the limb ranges the next cube relies on, and the derived column bounds
themselves (every carry taken in 32 bits), on 10^5 random inputs and the corners of each caller's
range.  No GPU, no library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "pm_carry_test")


def _binary():
    if not os.path.exists(BIN):  # host-only build of mont26.h (zk-lisp_amd/Makefile)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "zk-lisp_amd"), "../tests/cpp/pm_carry_test"], check=True)
    return BIN


def test_cube_and_fold_match_reference_and_bounds():
    r = subprocess.run([_binary(), "100000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "ok pm carry: 100000 random inputs" in r.stdout
    m = re.search(r"max carry fold (\d+) top (\d+)", r.stdout)
    # the bounds of mont26.h: a fold column's carry < 2^22 (so certainly < 2^32), top < 2^16; and
    # the corners do reach the neighbourhood of the bound (a bound nothing approaches tests nothing)
    assert (1 << 21) < int(m.group(1)) < (1 << 22)
    assert (1 << 15) < int(m.group(2)) < (1 << 16)
