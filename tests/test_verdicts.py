"""The verifiers answer a damaged proof with the same message as before the proof codec was
shared (zk-lisp_amd/csrc/proof_codec.h): tests/golden/verdicts.json holds, for a corpus of
mutations of an oracle segment proof and of two aggregation artifacts (base field and quadratic
extension), the message zkl_verify_segment / zkl_agg_verify gave at the commit named in each
entry; tests/golden/make_verdicts.py describes the corpus and rebuilds the proofs.  Host code,
no GPU."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_verdicts  # noqa: E402


def test_every_recorded_verdict_is_reproduced(oracle):
    gold = json.load(open(os.path.join(HERE, "golden", "verdicts.json")))
    proofs = make_verdicts.base_proofs()
    assert set(proofs) == set(gold["proofs"]) == {"segment", "agg_ext1", "agg_ext2"}
    for name, (b, verify) in proofs.items():
        assert hashlib.sha256(b).hexdigest() == gold["proofs"][name]["sha256"], name
        assert verify(b) == "", name
        # the fixture is the corpus the generator describes, entry for entry
        want = [(label, ops) for label, ops in make_verdicts.mutations(b)]
        assert [(e["mutation"], e["ops"]) for e in gold["entries"] if e["proof"] == name] == want, name
    assert len(gold["entries"]) > 600
    wrong = []
    for e in gold["entries"]:
        b, verify = proofs[e["proof"]]
        got = verify(make_verdicts.apply(b, e["ops"]))
        if got != e["message"]:
            wrong.append((e["proof"], e["mutation"], e["message"], got))
    assert not wrong, f"{len(wrong)} of {len(gold['entries'])} verdicts changed; first: {wrong[0]}"
