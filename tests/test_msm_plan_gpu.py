"""The batch plan of the fixed-base MSM (csrc/msm.hip msm_plan) on both sides of every threshold:
the header plk_debug_msm_snapshot reports (B, chunk, rb, fb, NC, NR, G, nbits, nout, the sort
path, the strides, the task bound, ...) equals, field for field, the one recorded in
tests/golden/msm_plan_headers.json with the library of the commit named there
(tools/record_msm_plan.py: the shapes, and which threshold each pair straddles). Integers only,
no tolerance; `gen` is not recorded."""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import record_msm_plan as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = json.loads(R.GOLDEN.read_text())


def test_fixture_covers_the_cases(plk):
    assert sorted(GOLDEN["cases"]) == sorted(R.CASES)
    assert GOLDEN["seed"] == R.SEED and len(GOLDEN["recorded_at_commit"]) >= 7
    fields = sorted(set(plk.plonk.MSM_SNAPSHOT_HDR) - {"gen"})
    assert all(sorted(h) == fields for h in GOLDEN["cases"].values())


def test_fixture_straddles_the_thresholds():
    """The recorded headers themselves show each threshold's two sides."""
    g = GOLDEN["cases"]
    assert (g["c13_len8192"]["hold"], g["c13_len8192"]["chunk"]) == (1, 8)
    assert (g["c13_len8193"]["hold"], g["c13_len8193"]["chunk"]) == (0, 16)
    assert g["c13_len32768"]["sort_one"] == 1 and g["c13_len32769"]["sort_one"] == 0
    assert g["c13_len1024"]["B"] == 4096 and g["c14_len1024"]["B"] == 8192
    assert g["c16_len256"]["wide"] == 0 and g["c17_len256"]["wide"] == 1
    assert [g[f"c{c}_len256"]["rb"] for c in (17, 20, 22)] == [1, 3, 4]
    assert [g[f"c{c}_2slots"]["rb"] for c in (17, 20, 22)] == [4, 4, 4]
    assert g["c17_len256"]["fb"] == 10
    assert {g[f"c17_part{p}of2"]["fb"] for p in range(2)} == {9}
    assert {g[f"c17_part{p}of4"]["fb"] for p in range(4)} == {8}
    assert g["c10_16x16384"]["chunk"] == 26


@pytest.mark.parametrize("name", list(R.CASES))
def test_header_equals_the_recorded_one(plk, gpu_ctx, name):
    assert R.case_header(plk, gpu_ctx, name) == GOLDEN["cases"][name]
