"""The column sum over G1 (csrc/g1_colsum.hip) through plk_debug_g1_colsum: out[t] = sum over the
rows of column t, against oracle/pyref.py's additions, bit for bit.

The launcher splits the rows of a column over min(rows, 64, ceil(65536 / cols)) lanes and sums the
partial sums in a second pass; with one row the first pass writes the result itself. Rows 1 (no
second pass), 2 and 3 (every lane one row), 64 (the widest split, one row a lane), 65 and 130 (64
lanes, lane 0 — and at 130 lanes 0 and 1 — with a second and third row). Columns 1, 63, 64, 65, 130:
less than a wave, one wave exactly, one more, and three blocks of the kernel.

The first columns are the exceptional cases of the group law — the sum must be the complete one,
since a prover who knows tau can make the products of one column coincide: P + P, P - P followed by
more terms, only identities, the identity first and last, one point repeated in every row, points
of the curve outside G1 (among them the point (0, 2) of order 3)."""
import functools

import numpy as np
import pytest

import g1_ingest_ref as G
import kzg_ref as K
import pyref as P

pytestmark = pytest.mark.gpu

R = P.R_MOD
ROWS = [1, 2, 3, 64, 65, 130]
COLS = [1, 63, 64, 65, 130]


@functools.lru_cache(maxsize=None)
def pool():
    """Affine points (None: the identity): 300 of G1 and 8 of the curve outside it."""
    rng = P.SplitMix64(31337)
    nrng = np.random.default_rng(5)
    pts = K.gen_mul_many([rng.fr() for _ in range(300)])
    out = [G.random_curve_point(nrng) for _ in range(6)] + [(0, 2), G.non_member(11, nrng)]
    assert all(P.g1_is_on_curve(q) and not G.in_subgroup(q) for q in out)
    return pts, out


def matrix(rows: int, cols: int):
    """rows x cols affine points, row-major."""
    pts, outside = pool()
    rng = np.random.default_rng(1000 * rows + cols)
    m = [[pts[int(rng.integers(len(pts)))] for _ in range(cols)] for _ in range(rows)]
    p, q = pts[0], pts[1]
    fill = [pts[int(rng.integers(len(pts)))] for _ in range(rows)]
    special = [
        lambda a: p,                                              # one point in every row: P + P, then on
        lambda a: (p, P.g1_neg(p))[a] if a < 2 else fill[a],      # P - P followed by more terms
        lambda a: None,                                           # only identities
        lambda a: None if a in (0, rows - 1) else fill[a],        # the identity first and last
        lambda a: outside[a % len(outside)],                      # outside G1
        lambda a: (0, 2),                                         # order 3: P + P = -P, P + P + P = O
        lambda a: (q, q, P.g1_neg(q))[a % 3],                     # doubles, then cancels
        lambda a: p if a % 2 == 0 else P.g1_neg(p),               # every pair cancels
    ]
    for t, fn in enumerate(special):
        if t < cols:
            col = [fn(a) for a in range(rows)]
            for a in range(rows):
                m[a][t] = col[a]
    if cols == 1:  # the single column takes a case of its own per row count
        col = [special[rows % len(special)](a) for a in range(rows)]
        for a in range(rows):
            m[a][0] = col[a]
    return m


def column_sums(m):
    cols = len(m[0])
    acc = [(1, 1, 0)] * cols
    for row in m:
        acc = [P.jac_add(s, P.jac_from_affine(pt)) for s, pt in zip(acc, row)]
    return [P.jac_to_affine(s) for s in acc]


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_column_sum_matches_the_reference_additions(plk, gpu_ctx, rows, cols):
    m = matrix(rows, cols)
    flat = P.g1_vec_to_np([pt for row in m for pt in row])
    got = plk.debug_g1_colsum(flat, rows, cols, gpu_ctx)
    assert np.array_equal(got, P.g1_vec_to_np(column_sums(m)))


def test_exceptional_columns_give_what_they_should(plk, gpu_ctx):
    rows, cols = 4, 8
    m = matrix(rows, cols)
    p = pool()[0][0]
    got = plk.debug_g1_colsum(P.g1_vec_to_np([pt for row in m for pt in row]), rows, cols, gpu_ctx)
    ident = P.g1_vec_to_np([None])[0]
    assert np.array_equal(got[0], P.g1_vec_to_np([P.g1_mul(p, 4)])[0])
    assert np.array_equal(got[2], ident) and np.array_equal(got[7], ident)
    assert np.array_equal(got[5], P.g1_vec_to_np([(0, 2)])[0])  # 4 (0, 2) = (0, 2)


def test_colsum_arguments(plk, gpu_ctx):
    lib, ptr = plk.plonk._lib(), plk.plonk._ptr
    pts = P.g1_vec_to_np([P.G1_GEN] * 6)
    out = np.zeros((6, 13), dtype=np.uint64)
    assert lib.plk_debug_g1_colsum(None, ptr(pts), 2, 3, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_colsum(gpu_ctx.handle, None, 2, 3, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_colsum(gpu_ctx.handle, ptr(pts), 0, 3, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_colsum(gpu_ctx.handle, ptr(pts), 2, 0, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_g1_colsum(gpu_ctx.handle, ptr(pts), 1 << 11, 1 << 11, ptr(out)) == plk.PLK_E_ARG
    bad = pts.copy()
    bad[4, 6] ^= np.uint64(1)  # off the curve
    assert lib.plk_debug_g1_colsum(gpu_ctx.handle, ptr(bad), 2, 3, ptr(out)) == plk.PLK_E_ARG
