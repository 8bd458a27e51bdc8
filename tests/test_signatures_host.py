"""The public interface of the binding and of the modules that upload host arrays, against tests/golden/context_signatures.json
(tools/gen_golden_signatures.py wrote it before the array marshalling moved into beat_amd._marshal)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_public_signatures_unchanged():
    import gen_golden_signatures
    with open(os.path.join(ROOT, "tests", "golden", "context_signatures.json")) as fh:
        golden = json.load(fh)
    now = gen_golden_signatures.signatures()
    assert len(golden["engine.Context"]) == 115
    assert sorted(now) == sorted(golden)
    for owner in golden:
        assert now[owner] == golden[owner], owner
