"""The pairing's tower one operation at a time on the device (k_f12_op and k_miller_value of
csrc/pairing.hip: csrc/pairing.hpp over the wave-tiled F12Dev workspace k_pairing uses) at 1, 64,
65 and 130 rows: one lane, a full wave, one lane over, and three tiles with a partial last one.
Structured operands sit at lanes 0, 63, 64 and the last one (and on from lane 1 until they are
all placed), random ones elsewhere. Every row equals the host code's (the same source over a
plain array: what differs is the slot store and what the compiler kept in registers across
f12_fence), and the structured rows and a sample of the random ones equal the big-integer
restatement. All comparisons are exact.
"""
import numpy as np
import pytest

import g1_ingest_ref as ref
import pairing_ref as R
import pairing_tower_ops as T
import pyref as P
from make_pairing_tower_vectors import OUT
from make_pairing_vectors import OUT as PAIRING_OUT
from make_pairing_vectors import f12_from_row, g2_row

pytestmark = pytest.mark.gpu

COUNTS = [1, 64, 65, 130]
TAU = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99


def lanes(n):
    """Where the structured operands go, in order: ABI_LANES and the last lane, then 1, 2, .."""
    first = [k for k in (*ref.ABI_LANES, n - 1) if k < n]
    first = list(dict.fromkeys(first))
    return first + [k for k in range(n) if k not in first]


def place(n, structured, filler, shift=0):
    """n operands: `structured` (rotated by `shift`) on lanes(n) as far as it goes, `filler`
    elsewhere. Returns (operands, the lanes that hold a structured one)."""
    structured = structured[shift % len(structured):] + structured[:shift % len(structured)]
    out = list(filler[:n])
    assert len(out) == n
    where = lanes(n)[:len(structured)]
    for k, s in zip(where, structured):
        out[k] = s
    return out, where


def sample(n, where, extra=3):
    """The rows compared with the restatement: the structured ones and a few others."""
    rest = [k for k in range(n) if k not in where]
    return list(where) + rest[:: max(1, len(rest) // extra)][:extra]


@pytest.fixture(scope="module")
def pool():
    """130 random Fp12 elements, twice (computed once, never changed)."""
    return T.rand_f12(130, 0x6A), T.rand_f12(130, 0x6B)


@pytest.fixture(scope="module")
def tower():
    return dict(np.load(OUT, allow_pickle=False))


@pytest.fixture(scope="module")
def vec():
    return dict(np.load(PAIRING_OUT, allow_pickle=False))


def both(plk, gpu_ctx, op, a, b=None, **kw):
    """The op on the device, asserted equal to the host's on every row -> the rows."""
    got = plk.debug_f12_op(op, a, b, ctx=gpu_ctx, **kw)
    assert np.array_equal(got, plk.debug_f12_op(op, a, b, **kw)), op
    return got


# ---- Fp2 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_f2_ops(plk, gpu_ctx, n):
    ops = T.pack_f2(T.f2_operands())
    core = T.f2_core()
    xs = T.pack_f2([x for x in core for _ in core])
    ys = T.pack_f2([y for _ in core for y in core])
    fill_a, fill_b = T.rand_f12(n, 0x21), T.rand_f12(n, 0x22)
    a, where = place(n, ops, fill_a, shift=n)
    rows_a = T.rows(a)
    for op in ("f2_sqr", "f2_inv", "f2_mul_xi"):
        got = T.unrows(both(plk, gpu_ctx, op, rows_a))
        for k in sample(n, where):
            assert got[k] == T.expected(op, a[k]), (op, k)
    a, where = place(n, xs, fill_a, shift=n)
    b, _ = place(n, ys, fill_b, shift=n)
    got = T.unrows(both(plk, gpu_ctx, "f2_mul", T.rows(a), T.rows(b)))
    for k in sample(n, where):
        assert got[k] == T.expected("f2_mul", a[k], b[k]), k


# ---- Fp12 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_mul_and_sqr(plk, gpu_ctx, pool, n):
    s = T.f12_operands(0)
    a, where = place(n, s, pool[0], shift=n)
    b, _ = place(n, s, pool[1], shift=3 * n + 1)  # another structured partner on every lane
    ra, rb = T.rows(a), T.rows(b)
    got = T.unrows(both(plk, gpu_ctx, "mul", ra, rb))
    for k in sample(n, where):
        assert got[k] == R.f12mul(a[k], b[k]), k
    sq = both(plk, gpu_ctx, "sqr", ra)
    assert np.array_equal(sq, plk.debug_f12_op("mul", ra, ra, ctx=gpu_ctx))
    got = T.unrows(sq)
    for k in sample(n, where):
        assert got[k] == R.f12sqr(a[k]), k


@pytest.mark.parametrize("n", COUNTS)
def test_mul_line(plk, gpu_ctx, pool, n):
    lines = T.line_operands()
    special = lines[len(T.EDGES):] + lines[:len(T.EDGES)]  # the zero-coefficient lines first
    filler = [lines[-1 - k % 4] for k in range(n)]
    ln, where = place(n, special, filler, shift=0)
    a, _ = place(n, T.f12_operands(0), pool[0], shift=n + 2)
    got = T.unrows(both(plk, gpu_ctx, "mul_line", T.rows(a), np.stack([T.line_row(*l) for l in ln])))
    for k in sample(n, where):
        assert got[k] == R.f12mul(a[k], R.line(*ln[k])), k


@pytest.mark.parametrize("n", COUNTS)
def test_conj_and_frobenius(plk, gpu_ctx, pool, n):
    a, where = place(n, T.f12_operands(0), pool[0], shift=2 * n)
    ra = T.rows(a)
    for op in ("conj", "frob1", "frob2"):
        out = both(plk, gpu_ctx, op, ra)
        assert np.array_equal(out, both(plk, gpu_ctx, op, ra, in_place=True)), op
        got = T.unrows(out)
        # the literal powers cost ~0.1 s each: the four pinned lanes and one random row
        for k in (where[:4] + [k for k in range(n) if k not in where][:1]):
            assert got[k] == T.expected(op, a[k]), (op, k)


@pytest.mark.parametrize("n", COUNTS)
def test_inv_even(plk, gpu_ctx, pool, n):
    a, where = place(n, T.f12_operands(0), pool[0], shift=n + 5)  # odd coefficients: not read
    got = T.unrows(both(plk, gpu_ctx, "inv_even", T.rows(a)))
    for k in sample(n, where):
        even = [x if i % 2 == 0 else (0, 0) for i, x in enumerate(a[k])]
        assert all(got[k][i] == (0, 0) for i in (1, 3, 5)), k
        assert R.f12mul(even, got[k]) == (R.F12_ZERO if even == R.F12_ZERO else R.F12_ONE), k


@pytest.mark.parametrize("n", COUNTS)
def test_cyc_sqr(plk, gpu_ctx, vec, n):
    special = [list(R.F12_ONE)] + [f12_from_row(v) for v in vec["value"]]
    special.append(R.f12conj(special[4]))
    a, where = place(n, special, T.cyclotomic(130), shift=n)
    ra = T.rows(a)
    out = both(plk, gpu_ctx, "cyc_sqr", ra)
    assert np.array_equal(out, plk.debug_f12_op("sqr", ra, ctx=gpu_ctx))
    got = T.unrows(out)
    for k in sample(n, where):
        assert got[k] == R.f12mul(a[k], a[k]), k


@pytest.mark.parametrize("n", COUNTS)
def test_final_exp(plk, gpu_ctx, tower, pool, n):
    cases = len(tower["input"])
    a = T.rows(pool[0][:n])
    where = lanes(n)[:cases]
    shift = n % cases
    order = [(shift + i) % cases for i in range(len(where))]
    for k, c in zip(where, order):
        a[k] = tower["input"][c]
    got = both(plk, gpu_ctx, "final_exp", a)
    for k, c in zip(where, order):
        assert np.array_equal(got[k], tower["value"][c]), (k, c)


# ---- the Miller value -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1_pool(vec):
    """130 points of G1, and the structured ones: G, the fixture's wide-x point, (0, 2), infinity."""
    pts = [P.g1_mul(P.G1_GEN, k) for k in range(2, 132)]
    special = [T.T3, None, P.g1_vec_from_np(vec["p"][6:7])[0], P.G1_GEN]
    return pts, special


@pytest.mark.parametrize("n", COUNTS)
def test_miller_one_pair(plk, gpu_ctx, g1_pool, n):
    pts, where = place(n, g1_pool[1], g1_pool[0], shift=n)
    rows, h = T.g1_rows(pts), g2_row(R.G2_GEN)
    got = plk.debug_miller(rows, h, ctx=gpu_ctx)
    assert np.array_equal(got, plk.debug_miller(rows, h))
    got = T.unrows(got)
    for k in sample(n, where):
        assert got[k] == R.miller_loop(pts[k], R.G2_GEN), k


@pytest.mark.parametrize("n", COUNTS)
def test_miller_two_pairs(plk, gpu_ctx, g1_pool, n):
    q0, q1 = R.G2_GEN, R.g2_mul(R.G2_GEN, TAU)
    p0, where = place(n, g1_pool[1], g1_pool[0], shift=n)
    # the partner on the pinned lanes: (T, O), (O, O), (wide, T), (G, T) in some rotation; then
    # lanes with an infinite or order-3 second point next to a finite first one
    p1, where1 = place(n, [None, None, T.T3, T.T3, None, T.T3], g1_pool[0][::-1], shift=n)
    r0, r1 = T.g1_rows(p0), T.g1_rows(p1)
    got = plk.debug_miller(r0, g2_row(q0), r1, g2_row(q1), ctx=gpu_ctx)
    assert np.array_equal(got, plk.debug_miller(r0, g2_row(q0), r1, g2_row(q1)))
    got = T.unrows(got)
    for k in sample(n, sorted(set(where) | set(where1))):
        assert got[k] == T.miller_pair(p0[k], q0, p1[k], q1), k
