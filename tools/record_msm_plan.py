"""Records tests/golden/msm_plan_headers.json: the header plk_debug_msm_snapshot reports (the
batch plan of csrc/msm.hip msm_plan, the workspace strides) for a table of shapes with one on
each side of every threshold of the plan. tests/test_msm_plan_gpu.py recomputes the headers and
asserts equality field for field.

    PLK_LIB=<libplk.so of the commit being recorded> PLK_LIB_ANY_SRC=1 \\
        python tools/record_msm_plan.py --commit <its id>

Run on a GPU with the library of the commit whose behaviour is the reference (the parent of a
refactor): the file is never re-recorded to make a test pass. `gen` (the workspace's batch
counter) is left out of the record.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

GOLDEN = ROOT / "tests" / "golden" / "msm_plan_headers.json"
SEED = 0x91A7


def _case(c, n_srs, lens, **kw):
    return {"c": c, "n_srs": n_srs, "lens": list(lens), **kw}


# 16 unequal slots, one of them empty
UNEQUAL16 = [16384, 0, 1, 63, 64, 65, 1000, 1024, 4095, 4096, 8192, 8193, 12000, 15000, 16383, 7]

# name -> shape: the SRS (window size c forced, n_srs points), the slots' lengths and the
# snapshot's options (tail_quad, shared_chip, part, parts). At most 40 000 scalars per slot and
# 2^16 SRS points.
CASES = {
    # kSortOneMax: the scalars held in registers or not, chunk floor 8 -> 16
    "c13_len8192": _case(13, 32769, [8192]),
    "c13_len8193": _case(13, 32769, [8193]),
    # kSortOneBig: one-dispatch sort -> histogram + k_sort_small
    "c13_len32768": _case(13, 32769, [32768]),
    "c13_len32769": _case(13, 32769, [32769]),
    # kSortSmallMax: 4096 / 8192 buckets
    "c13_len1024": _case(13, 32769, [1024]),
    "c14_len1024": _case(14, 1024, [1024]),
    # kLdsBuckets: narrow / wide
    "c16_len256": _case(16, 256, [256]),
    "c17_len256": _case(17, 256, [256]),
    # run_bits of a lone MSM: rb clamps at 1, 3, 4
    "c20_len256": _case(20, 256, [256]),
    "c22_len256": _case(22, 256, [256]),
    # run_bits of a batch: rb = 4
    "c17_2slots": _case(17, 256, [256, 255]),
    "c20_2slots": _case(20, 256, [256, 255]),
    "c22_2slots": _case(22, 256, [256, 255]),
    # bucket-range parts: fb 10 / 9 / 8 (parts = 1 is c17_len256)
    **{f"c17_part{p}of{n}": _case(17, 256, [256], part=p, parts=n) for n in (2, 4) for p in range(n)},
    # chunk_fit above its floor (26), and unequal batches with an empty slot
    "c10_16x16384": _case(10, 16384, [16384] * 16),
    "c10_2slots_unequal": _case(10, 16384, [5000, 0]),
    "c10_16slots_unequal": _case(10, 16384, UNEQUAL16),
    # tail_quad 0 / 1 / 2 and shared_chip 0 / 1, narrow and wide (tail_quad = 1, lone: the defaults above)
    "c13_len1024_tail0": _case(13, 32769, [1024], tail_quad=0),
    "c13_len1024_tail2": _case(13, 32769, [1024], tail_quad=2),
    "c17_len256_tail0": _case(17, 256, [256], tail_quad=0),
    "c17_len256_tail2": _case(17, 256, [256], tail_quad=2),
    "c13_len1024_shared": _case(13, 32769, [1024], shared_chip=True),
    "c17_len256_shared": _case(17, 256, [256], shared_chip=True),
}


def case_header(plk, ctx, name: str) -> dict:
    """The snapshot header of one case (without `gen`), computed in this process."""
    from oracle_lib import random_fr
    from test_msm_stage_gpu import tau_srs
    case = dict(CASES[name])
    c, n_srs, lens = case.pop("c"), case.pop("n_srs"), case.pop("lens")
    pp, _ = tau_srs(plk, ctx, c, n_srs)
    slots = [random_fr(n, seed=SEED + 31 * k + n) if n else np.zeros((0, 4), np.uint64)
             for k, n in enumerate(lens)]
    h, _ = plk.plonk.debug_msm_snapshot(pp, slots, points=False, **case)
    h.pop("gen")
    return h


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="id of the commit being recorded (noted in the file)")
    ap.add_argument("--out", default=str(GOLDEN))
    a = ap.parse_args()
    import dusk_plonk_amd as plk
    if plk.device_count() == 0:
        raise SystemExit("no GPU visible")
    ctx = plk.Context.default(0)
    cases = {name: case_header(plk, ctx, name) for name in CASES}
    doc = {"recorded_at_commit": a.commit, "seed": SEED, "cases": cases}
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {a.out}: {len(cases)} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
