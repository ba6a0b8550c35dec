"""Generates tests/golden/verdicts.json: what zkl_verify_segment / zkl_agg_verify answer, message
for message, to a corpus of damaged proofs (tests/test_verdicts.py holds the library to it).

Three proofs, all made by the oracle (oracle/prover.c, oracle/agg_ref.py):
  * "segment": a 64-row segment proof (synth_segment(0x5EED0B10, 6, 0), queries 16, blowup 8,
    grind 2: the shape tests/test_verifier.py uses);
  * "agg_ext1" / "agg_ext2": the aggregation artifact of 2 children at FieldExtension::None and
    ::Quadratic; the mutations are applied to the ZlAggAir proof inside the artifact, whose
    length field is rewritten to match.

Mutations (each an entry: the proof, a label, edit operations, the message, "" for accept):
  * truncation at every section boundary (length prefix, payload start, payload end) and one
    byte either side of it; one appended byte;
  * each of the 34 context bytes set to 0xFF and to 0x00 (where that changes it);
  * the FRI layer count +-1; the FRI partitions byte set to 1;
  * the length prefix of each of the six query / OOD slices +-1;
  * an all-ones (non-canonical) element at the start and at the end of every value section;
  * 64 seeded single-bit flips.
Edit operations: ["trunc", n] keeps the first n bytes, ["splice", off, k, hex] replaces k bytes
at off by the given ones, ["xor", off, mask].

"parent" is the commit whose library gave the messages.  Run with that commit built:
    python tests/golden/make_verdicts.py
"""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "verdicts.json")
AGG_PROGRAM = 0x5EEDA9C0
CONTEXT_LEN = 34  # TraceInfo 6, element size 1, modulus 16, ProofOptions 10, num_unique_queries 1


def _imports():
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "zk-lisp_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import agg_ref
    import oracle_lib
    import zkl_hip
    oracle_lib.build()
    return oracle_lib, agg_ref, zkl_hip


def base_proofs():
    """{name: (bytes the mutations edit, verify(bytes) -> message)}"""
    oracle, agg_ref, zkl_hip = _imports()

    def message(f, *a):
        try:
            f(*a)
            return ""
        except zkl_hip.ZklError as e:
            return str(e)

    out = {}
    n = 64
    t, opi, w = oracle.synth_segment(0x5EED0B10, 6, 0)
    oo = oracle.default_options(w, n, queries=16, blowup=8, grind=2)
    proof = oracle.prove(t, w, n, opi, oo)
    pi = zkl_hip.AirPublicInputs()
    C.memmove(C.byref(pi), C.byref(opi), C.sizeof(pi))
    o = zkl_hip.ProofOptions(*[getattr(oo, f) for f, _ in oo._fields_])
    out["segment"] = (proof, lambda b: message(zkl_hip.verify_segment, b, pi, o))

    steps, rom0 = [], 0
    for i in range(2):
        t, cpi, w = oracle.synth_segment_chain(AGG_PROGRAM, AGG_PROGRAM + i, 5, rom0, 0)
        inner = oracle.prove(t, w, 32, cpi, oracle.default_options(w, 32, queries=8, grind=4))
        zpi = zkl_hip.AirPublicInputs()
        C.memmove(C.byref(zpi), C.byref(cpi), C.sizeof(zpi))
        info = zkl_hip.step_info_for(zpi, i, 2, i.to_bytes(32, "little"), (i + 1).to_bytes(32, "little"))
        steps.append(zkl_hip.step_proof_encode(zpi, info, inner))
        rom0 = cpi.rom_s_out[0].lo | (cpi.rom_s_out[0].hi << 64)
    for ext, bits in ((1, 64), (2, 128)):
        art, _, _ = agg_ref.agg_prove(oracle, steps, queries=64, blowup=16, grind=8, min_security_bits=bits)
        inner = zkl_hip.parse_agg_artifact(art)["proof"]
        head = art[:len(art) - len(inner) - 4]
        assert art == head + len(inner).to_bytes(4, "little") + inner

        def verify(b, head=head, bits=bits):
            return message(zkl_hip.agg_verify, head + len(b).to_bytes(4, "little") + b, bits)
        out[f"agg_ext{ext}"] = (inner, verify)
    return out


def read_vint(b, off):
    """winter-utils read_usize: (value, encoded length)"""
    if b[off] == 0:
        return int.from_bytes(b[off + 1:off + 9], "little"), 9
    ln = (b[off] & -b[off]).bit_length()
    return int.from_bytes(b[off:off + ln], "little") >> ln, ln


def write_vint(x):
    lz = 64 - x.bit_length()
    ln = 9 - min((lz - 1) // 7 if lz > 0 else 0, 8)
    if ln == 9:
        return b"\0" + x.to_bytes(8, "little")
    return ((((x << 1) | 1) << (ln - 1)) & ((1 << (8 * ln)) - 1)).to_bytes(ln, "little")


def sections(b):
    """[(name, start, payload start, end)] of Proof::to_bytes"""
    out = [("context", 0, 0, CONTEXT_LEN)]
    off = CONTEXT_LEN

    def vec(name):
        nonlocal off
        v, ln = read_vint(b, off)
        out.append((name, off, off + ln, off + ln + v))
        off += ln + v

    def plain(name, k):
        nonlocal off
        out.append((name, off, off, off + k))
        off += k

    vec("commitments")
    plain("trace_segments", 1)
    for name in ("trace_values", "trace_paths", "constraint_values", "constraint_paths", "ood_trace", "ood_constraints"):
        vec(name)
    layers = read_vint(b, off)[0]
    plain("fri_layer_count", read_vint(b, off)[1])
    for d in range(layers):
        vec(f"fri_values_{d}")
        vec(f"fri_paths_{d}")
    vec("remainder")
    plain("fri_partitions", 1)
    plain("nonce", 8)
    assert off == len(b)
    return out


def mutations(b):
    """[(label, ops)] for the proof bytes b"""
    sec = sections(b)
    by = {s[0]: s for s in sec}
    out = []
    for at in sorted({x for s in sec for x in s[1:]}):
        for k in (at - 1, at, at + 1):
            if 0 <= k < len(b):
                out.append((f"truncate to {k}", [["trunc", k]]))
    out.append(("append a byte", [["splice", len(b), 0, "00"]]))
    for i in range(CONTEXT_LEN):
        for v in (0xFF, 0x00):
            if b[i] != v:
                out.append((f"context byte {i} = {v:#04x}", [["splice", i, 1, f"{v:02x}"]]))
    _, at, _, end = by["fri_layer_count"]
    layers = read_vint(b, at)[0]
    for d in (-1, 1):
        out.append((f"fri layer count {d:+d}", [["splice", at, end - at, write_vint(layers + d).hex()]]))
    out.append(("fri partitions byte = 1", [["splice", by["fri_partitions"][1], 1, "01"]]))
    for name in ("trace_values", "trace_paths", "constraint_values", "constraint_paths", "ood_trace", "ood_constraints"):
        _, at, pay, end = by[name]
        for d in (-1, 1):
            out.append((f"{name} length {d:+d}", [["splice", at, pay - at, write_vint(end - pay + d).hex()]]))
    for name, _, pay, end in sec:
        if name in ("trace_values", "constraint_values", "ood_trace", "ood_constraints", "remainder") or name.startswith("fri_values"):
            out.append((f"{name}: first element all ones", [["splice", pay, 16, "ff" * 16]]))
            out.append((f"{name}: last element all ones", [["splice", end - 16, 16, "ff" * 16]]))
    rng = random.Random(0x5EED7E5D)
    for _ in range(64):
        i, m = rng.randrange(len(b)), 1 << rng.randrange(8)
        out.append((f"flip bit {m:#04x} of byte {i}", [["xor", i, m]]))
    return out


def apply(b, ops):
    b = bytearray(b)
    for op in ops:
        if op[0] == "trunc":
            del b[op[1]:]
        elif op[0] == "splice":
            b[op[1]:op[1] + op[2]] = bytes.fromhex(op[3])
        elif op[0] == "xor":
            b[op[1]] ^= op[2]
        else:
            raise ValueError(op[0])
    return bytes(b)


def main():
    parent = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    proofs, entries = {}, []
    for name, (b, verify) in base_proofs().items():
        assert verify(b) == "", name
        proofs[name] = {"len": len(b), "sha256": hashlib.sha256(b).hexdigest()}
        for label, ops in mutations(b):
            entries.append({"proof": name, "mutation": label, "ops": ops, "message": verify(apply(b, ops)),
                            "parent": parent})
        print(name, len(b), "bytes,", sum(e["proof"] == name for e in entries), "entries,",
              sum(e["proof"] == name and e["message"] == "" for e in entries), "accepted", flush=True)
    json.dump({"proofs": proofs, "entries": entries}, open(OUT, "w"), indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
