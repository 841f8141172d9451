#!/usr/bin/env python3
"""Writes tests/golden/pairing_tower_vectors.npz from tests/pairing_ref.py (big integers only;
about ten seconds): the inputs of the final-exponentiation tests and their expected values, the
plain final power (p^12 - 1) / r cubed.

  input  uint64[7, 72]  Fp12 elements, plk_debug_pairing's row layout (Montgomery limbs)
  value  uint64[7, 72]  input^(3 (p^12 - 1) / r)

Cases, in the order of CASES: three random elements; one; an element of Fp6 (the easy part sends
it to one); the raw Miller value ML(P, H) of the pairing fixture's wide-x point P; zero (the
power of zero is zero, and so is the product's result by its inverse-of-zero convention).

  python tests/make_pairing_tower_vectors.py      # rewrites the fixture (committed)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent / "oracle"))
import pairing_ref as R  # noqa: E402
import pyref as P  # noqa: E402
import make_pairing_vectors as V  # noqa: E402

OUT = HERE / "golden" / "pairing_tower_vectors.npz"
CASES = ("random 0", "random 1", "random 2", "one", "Fp6", "Miller value", "zero")
SEED = 0x7F12E


def random_f12(rng):
    return [(_fp(rng), _fp(rng)) for _ in range(6)]


def _fp(rng):
    """A uniform value below p from seven 64-bit draws (2^448 / p > 2^66: no visible bias)."""
    v = 0
    for _ in range(7):
        v = (v << 64) | rng.next_u64()
    return v % R.p


def wide_point():
    """The pairing fixture's P whose x has all 381 bits significant (V.cases()[6])."""
    return P.g1_mul(P.G1_GEN, V.cases()[6][0])


def inputs():
    rng = P.SplitMix64(SEED)
    rnd = [random_f12(rng) for _ in range(4)]
    fp6 = [rnd[3][i] if i % 2 == 0 else (0, 0) for i in range(6)]
    return rnd[:3] + [list(R.F12_ONE), fp6, R.miller_loop(wide_point(), R.G2_GEN), list(R.F12_ZERO)]


def main():
    ins = inputs()
    assert len(ins) == len(CASES)
    vals = [R.final_power_cubed(f) for f in ins]
    np.savez(OUT, input=np.stack([V.f12_row(f) for f in ins]),
             value=np.stack([V.f12_row(v) for v in vals]))
    print(f"wrote {OUT.relative_to(HERE.parent)} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
