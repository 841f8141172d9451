"""The pairing's tower one operation at a time on the host (csrc/pairing.hpp over F12Host, through
plk_debug_f12_op(ctx = NULL) and plk_debug_miller(ctx = NULL)) against the big-integer
restatement tests/pairing_ref.py, bit for bit, at operands with structure: zero coefficients,
c0 == +-c1, components p - 1, subfield and line-shaped elements, zero itself. Needs no GPU.

Every reference value is derived another way than the product's formula: squares from the general
product, Frobenius maps as literal p-th powers, inverses from a polynomial gcd, the final
exponentiation as the plain power (p^12 - 1) / r cubed (fixture, one value recomputed here).
"""
import numpy as np
import pytest

import pairing_ref as R
import pairing_tower_ops as T
import pyref as P
from make_pairing_tower_vectors import CASES, OUT, inputs
from make_pairing_vectors import OUT as PAIRING_OUT
from make_pairing_vectors import f12_from_row, f12_row, g2_row

p = R.p
TAU = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99


@pytest.fixture(scope="module")
def tower():
    return dict(np.load(OUT, allow_pickle=False))


@pytest.fixture(scope="module")
def vec():
    return dict(np.load(PAIRING_OUT, allow_pickle=False))


def run(plk, op, a, b=None, **kw):
    """The host op on big-integer elements -> big-integer elements."""
    return T.unrows(plk.debug_f12_op(op, T.rows(a), None if b is None else T.rows(b), **kw))


# ---- the restatement's own new pieces -------------------------------------------------------------
def test_reference_inverse_and_frobenius():
    """f12inv a * a == 1 on random, sparse and subfield elements; the literal p-th power is the
    field automorphism (additive, fixes Fp) and p^6 is the conjugation."""
    for a in T.f12_operands(3):
        if a == R.F12_ZERO:
            assert R.f12inv(a) == R.F12_ZERO
        else:
            assert R.f12mul(a, R.f12inv(a)) == R.F12_ONE
    a, b = T.rand_f12(2, 0xF0)
    s = [R.f2add(x, y) for x, y in zip(a, b)]
    assert R.f12frob(s, 1) == [R.f2add(x, y) for x, y in zip(R.f12frob(a, 1), R.f12frob(b, 1))]
    assert R.f12frob(R.f12frob(R.f12frob(a, 2), 2), 2) == R.f12conj(a)
    c = R.easy_part(a)
    assert c != R.F12_ONE
    # in the cyclotomic subgroup: c^(p^4) c == c^(p^2)
    assert R.f12mul(R.f12frob(R.f12frob(c, 2), 2), c) == R.f12frob(c, 2)


def test_one_fixture_vector_recomputed(tower):
    """Keeps the fixture honest: the inputs from the seed, and case 1's value live."""
    ins = inputs()
    assert np.array_equal(T.rows(ins), tower["input"])
    assert np.array_equal(f12_row(R.final_power_cubed(ins[1])), tower["value"][1])


# ---- Fp2 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["f2_sqr", "f2_inv", "f2_mul_xi"])
def test_f2_unary(plk, op):
    a = T.pack_f2(T.f2_operands())
    assert run(plk, op, a) == [T.expected(op, x) for x in a]


def test_f2_inv_of_zero_is_zero(plk):
    assert run(plk, "f2_inv", [list(R.F12_ZERO)]) == [R.F12_ZERO]


def test_f2_mul(plk):
    core = T.f2_core()
    xs = [x for x in core for _ in core]
    ys = [y for _ in core for y in core]
    ops = T.f2_operands()
    xs += ops
    ys += ops[7:] + ops[:7]  # every operand against another one
    xs += ops
    ys += ops                # and against itself
    a, b = T.pack_f2(xs), T.pack_f2(ys)
    assert run(plk, "f2_mul", a, b) == [T.expected("f2_mul", x, y) for x, y in zip(a, b)]


# ---- Fp12 -------------------------------------------------------------------------------------------
def test_mul_every_pair(plk):
    s = T.f12_operands()
    a = [x for x in s for _ in s]
    b = [y for _ in s for y in s]
    assert run(plk, "mul", a, b) == [R.f12mul(x, y) for x, y in zip(a, b)]


def test_sqr(plk):
    s = T.f12_operands()
    got = run(plk, "sqr", s)
    assert got == [R.f12sqr(x) for x in s]
    assert got == run(plk, "mul", s, s)


def test_mul_line(plk):
    s, lines = T.f12_operands(), T.line_operands()
    a = [x for x in s for _ in lines]
    ln = [l for _ in s for l in lines]
    got = T.unrows(plk.debug_f12_op("mul_line", T.rows(a), np.stack([T.line_row(*l) for l in ln])))
    assert got == [R.f12mul(x, R.line(*l)) for x, l in zip(a, ln)]


def test_mul_line_ignores_the_rest_of_row_b(plk):
    """Only limbs 0..29 of row b are the line."""
    a = T.rand_f12(1, 0xAB)
    l = T.line_operands()[0]
    b = T.line_row(*l).reshape(1, 72).copy()
    b[0, 30:] = f12_row(T.rand_f12(1, 0xAC)[0])[30:]
    assert T.unrows(plk.debug_f12_op("mul_line", T.rows(a), b)) == [R.f12mul(a[0], R.line(*l))]


@pytest.mark.parametrize("op", ["conj", "frob1", "frob2"])
def test_conj_and_frobenius(plk, op):
    s = T.f12_operands(4)
    got = run(plk, op, s)
    assert got == [T.expected(op, x) for x in s]
    assert got == run(plk, op, s, in_place=True)


def test_inv_even(plk):
    s = [[x if i % 2 == 0 else (0, 0) for i, x in enumerate(e)] for e in T.f12_operands()]
    got = run(plk, "inv_even", s)
    for a, inv in zip(s, got):
        assert all(inv[i] == (0, 0) for i in (1, 3, 5))
        assert R.f12mul(a, inv) == (R.F12_ZERO if a == R.F12_ZERO else R.F12_ONE)
    assert got == [T.expected("inv_even", a) for a in s]
    assert run(plk, "inv_even", [list(R.F12_ZERO)]) == [R.F12_ZERO]
    # the odd coefficients of the operand are overwritten, never read
    assert run(plk, "inv_even", T.f12_operands()) == got


def test_cyc_sqr(plk, vec):
    s = T.cyclotomic(6) + T.cyclotomic(2, seed=0xC8) + [list(R.F12_ONE)]
    s += [f12_from_row(v) for v in vec["value"]]
    s.append(R.f12conj(f12_from_row(vec["value"][3])))
    for c in s[:2]:  # what the operands are: of order dividing p^4 - p^2 + 1
        assert R.f12mul(R.f12frob(R.f12frob(c, 2), 2), c) == R.f12frob(c, 2)
    got = run(plk, "cyc_sqr", s)
    assert got == [R.f12mul(x, x) for x in s]
    assert got == run(plk, "sqr", s)


def test_final_exp_equals_the_fixture(plk, tower):
    assert len(CASES) == len(tower["input"])
    got = plk.debug_f12_op("final_exp", tower["input"])
    for i, name in enumerate(CASES):
        assert np.array_equal(got[i], tower["value"][i]), name
    assert f12_from_row(got[CASES.index("one")]) == R.F12_ONE
    assert f12_from_row(got[CASES.index("Fp6")]) == R.F12_ONE
    assert f12_from_row(got[CASES.index("zero")]) == R.F12_ZERO


# ---- the Miller value -------------------------------------------------------------------------------
def wide_point(vec):
    return P.g1_vec_from_np(vec["p"][6:7])[0]


def test_miller_one_pair(plk, vec):
    pts = [P.G1_GEN, wide_point(vec), T.T3, None]
    assert P.g1_is_on_curve(T.T3) and P.g1_mul(T.T3, 3) is None
    for q in (R.G2_GEN, R.g2_mul(R.G2_GEN, TAU)):
        got = T.unrows(plk.debug_miller(T.g1_rows(pts), g2_row(q)))
        assert got == [R.miller_loop(pt, q) for pt in pts]
        assert got[3] == R.F12_ONE
    # and the value is what plk_debug_pairing raises to its power
    h = g2_row(R.G2_GEN)
    ml = plk.debug_miller(T.g1_rows(pts), h)
    assert np.array_equal(plk.debug_f12_op("final_exp", ml), plk.debug_pairing(T.g1_rows(pts), h))


def test_miller_two_pairs(plk, vec):
    q0, q1 = R.G2_GEN, R.g2_mul(R.G2_GEN, TAU)
    g, wide = P.G1_GEN, wide_point(vec)
    pairs = [(g, wide), (wide, g), (P.g1_mul(g, TAU), g), (T.T3, g), (g, T.T3), (T.T3, T.T3),
             (None, g), (g, None), (None, None), (T.T3, None)]
    got = T.unrows(plk.debug_miller(T.g1_rows([a for a, _ in pairs]), g2_row(q0),
                                    T.g1_rows([b for _, b in pairs]), g2_row(q1)))
    assert got == [T.miller_pair(a, q0, b, q1) for a, b in pairs]
    assert got[8] == R.F12_ONE


# ---- refusals ---------------------------------------------------------------------------------------
def test_refusals(plk):
    lib = plk.plonk._lib()
    a = T.rows(T.rand_f12(2, 1))
    out = np.zeros_like(a)
    ptr = plk.plonk._ptr

    def call(op, x, y, n):
        return lib.plk_debug_f12_op(None, op, None if x is None else ptr(x),
                                    None if y is None else ptr(y), n, ptr(out))

    ops = plk.plonk.F12_OPS
    assert call(ops["sqr"], a, None, 2) == plk.PLK_OK
    assert call(ops["sqr"], None, None, 2) == plk.PLK_E_ARG
    assert lib.plk_debug_f12_op(None, ops["sqr"], ptr(a), None, 2, None) == plk.PLK_E_ARG
    assert call(ops["sqr"], a, None, 0) == plk.PLK_E_ARG
    assert call(ops["sqr"], a, None, 4097) == plk.PLK_E_ARG
    assert call(13, a, None, 2) == plk.PLK_E_ARG
    assert call(-1, a, None, 2) == plk.PLK_E_ARG
    for name in ("mul", "f2_mul", "mul_line"):
        assert call(ops[name], a, None, 2) == plk.PLK_E_ARG
        assert call(ops[name], a, a, 2) == plk.PLK_OK
    for name in ("conj", "frob1", "frob2"):
        assert call(ops[name] | plk.plonk.F12_IN_PLACE, a, None, 2) == plk.PLK_OK
    assert call(ops["sqr"] | plk.plonk.F12_IN_PLACE, a, None, 2) == plk.PLK_E_ARG
    for k in (0, 11, 12 + 7):  # the limb rows c0 of w^0, c1 of w^5, and one of the second row
        bad = a.copy()
        bad.reshape(-1)[6 * k: 6 * k + 6] = P.int_to_limbs(p, 6)
        assert call(ops["sqr"], bad, None, 2) == plk.PLK_E_ARG
        assert call(ops["mul"], a, bad, 2) == plk.PLK_E_ARG
        assert call(ops["sqr"], a, bad, 2) == plk.PLK_OK  # b is not read


def test_miller_refusals(plk):
    lib = plk.plonk._lib()
    ptr = plk.plonk._ptr
    g = T.g1_rows([P.G1_GEN])
    h = g2_row(R.G2_GEN)
    out = np.zeros((1, 72), dtype=np.uint64)
    assert lib.plk_debug_miller(None, ptr(g), ptr(h), None, None, 1, ptr(out)) == plk.PLK_OK
    assert lib.plk_debug_miller(None, None, ptr(h), None, None, 1, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_miller(None, ptr(g), None, None, None, 1, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_miller(None, ptr(g), ptr(h), ptr(g), None, 1, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_miller(None, ptr(g), ptr(h), None, None, 0, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_miller(None, ptr(g), ptr(h), None, None, 4097, ptr(out)) == plk.PLK_E_ARG
    assert lib.plk_debug_miller(None, ptr(g), ptr(h), None, None, 1, None) == plk.PLK_E_ARG
    off = g.copy()
    off[0, 6] ^= np.uint64(1)
    inf = np.zeros(25, dtype=np.uint64)
    inf[24] = 1
    with pytest.raises(plk.PlonkError):
        plk.debug_miller(off, h)
    with pytest.raises(plk.PlonkError):
        plk.debug_miller(g, h, off, h)
    with pytest.raises(plk.PlonkError):
        plk.debug_miller(g, inf)
    with pytest.raises(plk.PlonkError):
        plk.debug_miller(g, h, g, inf)
