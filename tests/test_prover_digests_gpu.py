"""Key compilation, the commit paths and the prover hand out, bit for bit, what they did at the
commit tests/golden/prover_digests.json was recorded at (tools/record_prover_digests.py: the
cases, and why each size). Per case the SHA-256 of the proof bytes, of the key's 15 commitments
and of plk_debug_block_eval on a fixed 11-coefficient input are recomputed and compared: no
tolerance. The hot-wire case also compares commit_info(), the PLK_LAGRANGE_COMMIT=0 case runs in
a fresh child process (the variable is read at key compile), and the unsatisfied witness must be
refused with PLK_E_DEGREE and diagnosed as recorded."""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import record_prover_digests as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = json.loads(R.GOLDEN.read_text())


def test_fixture_covers_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(R.CASES)
    assert GOLDEN["seed"] == R.SEED and len(GOLDEN["recorded_at_commit"]) >= 7


@pytest.mark.parametrize("name", list(R.CASES))
def test_digests_equal_the_recorded_ones(plk, gpu_ctx, name):
    want = GOLDEN["cases"][name]
    got = R.case_record(plk, name)
    kind = R.CASES[name][2]
    if kind == "unsatisfied":
        assert want["status"] == plk.PLK_E_DEGREE and want["failing"] >= 1
    else:
        assert "proof" in want
    if kind == "hot":
        assert want["commit_basis"][1] == "coefficient"
    if kind == "lagrange_off":
        assert want["commit_basis"] == ["coefficient"] * 4
    assert got == want
