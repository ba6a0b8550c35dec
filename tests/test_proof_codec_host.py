"""The proof codec on the host (zk-lisp_amd/csrc/proof_codec.h) through the stand-alone program
tests/cpp/proof_codec_test: a synthetic proof written by ProofWriter and read back by the reader
steps field for field over both element widths, the reader's refusals, fold_positions against a
quadratic restatement on 10^4 seeded position sets and query_positions against sort + unique.
No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "proof_codec_test")


def _binary():
    if not os.path.exists(BIN):  # host-only build (zk-lisp_amd/Makefile)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "zk-lisp_amd"), "../tests/cpp/proof_codec_test"], check=True)
    return BIN


def test_round_trip_and_position_rules():
    r = subprocess.run([_binary(), "10000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "ok proof codec: round trip over both fields, 10000 position sets" in r.stdout
