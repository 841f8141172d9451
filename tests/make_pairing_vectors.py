#!/usr/bin/env python3
"""Writes tests/golden/pairing_vectors.npz from tests/pairing_ref.py (big integers only; about
ten seconds): eight (P, Q, value) triples with value = e(P, Q)^3, the plain final power
(p^12 - 1) / r cubed.

  p      uint64[8, 13]  G1 points, ABI layout (Montgomery limbs)
  q      uint64[8, 25]  G2 points, plk_g2 layout
  value  uint64[8, 72]  six Fp2 coefficients of w^0 .. w^5 as (c0, c1) Montgomery limbs
  a, b   uint64[8, 4]   the scalars: P = a G, Q = b H (plain little-endian limbs)

Cases: (G, H); a G and b H for random a, b in every combination; a small a; and one P whose x
coordinate has all 381 bits significant.

  python tests/make_pairing_vectors.py      # rewrites the fixture (committed)
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

OUT = HERE / "golden" / "pairing_vectors.npz"


def g2_row(q) -> np.ndarray:
    row = np.zeros(25, dtype=np.uint64)
    if q is None:
        row[24] = 1
        return row
    for k, v in enumerate((q[0][0], q[0][1], q[1][0], q[1][1])):
        row[6 * k: 6 * k + 6] = P.int_to_limbs(P.fp_to_mont(v), 6)
    return row


def f12_row(f) -> np.ndarray:
    row = np.zeros(72, dtype=np.uint64)
    for i, (c0, c1) in enumerate(f):
        row[12 * i: 12 * i + 6] = P.int_to_limbs(P.fp_to_mont(c0), 6)
        row[12 * i + 6: 12 * i + 12] = P.int_to_limbs(P.fp_to_mont(c1), 6)
    return row


def f12_from_row(row):
    return [(P.fp_from_mont(P.limbs_to_int(row[12 * i: 12 * i + 6])),
             P.fp_from_mont(P.limbs_to_int(row[12 * i + 6: 12 * i + 12]))) for i in range(6)]


def cases():
    rng = P.SplitMix64(0x9A1121)
    a, b = rng.fr(), rng.fr()
    a2, b2 = rng.fr(), rng.fr()
    wide = next(k for k in range(2, 1 << 12) if P.g1_mul(P.G1_GEN, k)[0].bit_length() == 381)
    return [(1, 1), (a, 1), (1, b), (a, b), (3, b2), (a2, b2), (wide, 1), (R.r - 1, b)]


def main():
    cs = cases()
    pts = [P.g1_mul(P.G1_GEN, a) for a, _ in cs]
    qs = [R.g2_mul(R.G2_GEN, b) for _, b in cs]
    assert any(pt[0].bit_length() == 381 for pt in pts)
    vals = [R.pairing_cubed(pt, q) for pt, q in zip(pts, qs)]
    np.savez(OUT,
             p=P.g1_vec_to_np(pts),
             q=np.stack([g2_row(q) for q in qs]),
             value=np.stack([f12_row(v) for v in vals]),
             a=np.array([P.int_to_limbs(a, 4) for a, _ in cs], dtype=np.uint64),
             b=np.array([P.int_to_limbs(b, 4) for _, b in cs], dtype=np.uint64))
    print(f"wrote {OUT.relative_to(HERE.parent)} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
