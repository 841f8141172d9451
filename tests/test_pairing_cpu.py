"""The host pairing (csrc/pairing.hpp through plk_debug_pairing(ctx = NULL), plk_pairing_check and
the opening key) against the big-integer restatement tests/pairing_ref.py. Needs no GPU.

Parity: the reference holds no pairing vector and its pairing crate is not vendored, so what is
pinned here is the mathematics: the values equal an independent big-integer pairing bit for bit,
and that pairing is bilinear, non-degenerate and of order r.
"""
import numpy as np
import pytest

import pairing_ref as R
import pairing_tower_ops as T
import pyref as P
from make_pairing_vectors import OUT, f12_from_row, f12_row, g2_row

r = P.R_MOD


@pytest.fixture(scope="module")
def vec():
    return dict(np.load(OUT, allow_pickle=False))


def scalars(rows):
    return [P.limbs_to_int(row) for row in rows]


def g1_words(pt):
    return P.g1_vec_to_np([pt])[0]


def pair_words(c, w):
    return np.stack([g1_words(c), g1_words(w)])


def test_host_values_equal_the_fixture(plk, vec):
    for i in range(8):
        got = plk.debug_pairing(vec["p"][i:i + 1], vec["q"][i])
        assert np.array_equal(got[0], vec["value"][i]), i


def test_one_fixture_vector_recomputed(vec):
    """Keeps the fixture honest: vector 3 (a G, b H) from the scalars alone."""
    a, b = scalars(vec["a"])[3], scalars(vec["b"])[3]
    pt, q = P.g1_mul(P.G1_GEN, a), R.g2_mul(R.G2_GEN, b)
    assert np.array_equal(P.g1_vec_to_np([pt])[0], vec["p"][3])
    assert np.array_equal(g2_row(q), vec["q"][3])
    assert np.array_equal(f12_row(R.pairing_cubed(pt, q)), vec["value"][3])


def test_bilinear_nondegenerate_order_r(plk, vec):
    """From the product's outputs: value(a G, b H) == value(G, H)^(a b); value(G, H) != 1 and
    its r-th power is 1."""
    out = plk.debug_pairing(vec["p"], vec["q"][0])  # every P against H ...
    base = f12_from_row(out[0])
    assert base != R.F12_ONE
    assert R.f12pow(base, r) == R.F12_ONE
    a, b = scalars(vec["a"]), scalars(vec["b"])
    for i in range(8):
        q_is_h = b[i] == 1
        got = f12_from_row(out[i] if q_is_h else plk.debug_pairing(vec["p"][i:i + 1], vec["q"][i])[0])
        assert got == R.f12pow(base, a[i] * b[i] % r), i


def test_infinity_is_the_factor_one(plk, vec):
    inf = g1_words(None)
    out = plk.debug_pairing(inf.reshape(1, 13), vec["q"][0])
    assert f12_from_row(out[0]) == R.F12_ONE
    key = plk.OpeningKey.setup(7)
    g = P.G1_GEN
    assert key.check(pair_words(None, None))
    assert not key.check(pair_words(g, None))
    assert not key.check(pair_words(None, g))


def test_check_accepts_and_rejects(plk):
    rng = P.SplitMix64(0xC0FFEE)
    tau, s = rng.fr(), rng.fr()
    key = plk.OpeningKey.setup(tau)
    w = P.g1_mul(P.G1_GEN, s)
    c = P.g1_mul(w, tau)
    assert key.check(pair_words(c, w))
    assert not key.check(pair_words(P.g1_add(c, P.G1_GEN), w))
    assert not key.check(pair_words(c, P.g1_neg(w)))
    # the same verdicts from the restatement
    h, bh = R.G2_GEN, R.g2_mul(R.G2_GEN, tau)
    assert R.pairing_check(c, w, h, bh)
    assert not R.pairing_check(P.g1_add(c, P.G1_GEN), w, h, bh)


def test_check_with_points_outside_the_subgroup(plk):
    """T = (0, 2) is on the curve, of order 3, and makes the line's w^2 coefficient zero. The
    check takes on-curve points without a subgroup test; its answer for pairs with T in them is
    the restatement's, and since T = r T' lies in r E the reduced pairing sends it to one: a
    commitment moved by T passes (DESIGN.md "Points outside G1")."""
    rng = P.SplitMix64(0x7033)
    tau, s = rng.fr(), rng.fr()
    key = plk.OpeningKey.setup(tau)
    h, bh = R.G2_GEN, R.g2_mul(R.G2_GEN, tau)
    answers = {}
    for name, (c, w) in T.off_subgroup_pairs(tau, P.g1_mul(P.G1_GEN, s)):
        assert P.g1_is_on_curve(c) and P.g1_is_on_curve(w), name
        answers[name] = key.check(pair_words(c, w))
        assert answers[name] == R.pairing_check(c, w, h, bh), name
    assert answers == {"(T, T)": True, "(C + T, W)": True, "(C, W + T)": True, "(T, O)": True,
                       "(tau (W + T), W + T)": True}


def test_check_refuses_malformed_points(plk):
    key = plk.OpeningKey.setup(5)
    g = g1_words(P.G1_GEN)
    off = g.copy()
    off[6] ^= np.uint64(1)
    big = g.copy()
    big[0:6] = P.int_to_limbs(P.P_MOD, 6)
    flag = g.copy()
    flag[12] = 2
    for bad in (off, big, flag):
        for pair in (np.stack([bad, g]), np.stack([g, bad])):
            with pytest.raises(plk.PlonkError) as err:
                key.check(pair)
            assert err.value.status == plk.PLK_E_ARG


def from_mont(row):
    return [P.fp_from_mont(P.limbs_to_int(row[6 * k: 6 * k + 6])) for k in range(4)]


def test_opening_key_round_trip_and_generator(plk):
    tau = 0x1234567890ABCDEF1234567890ABCDEF
    key = plk.OpeningKey.setup(tau)
    h, bh = key.points()
    (x, y) = R.G2_GEN
    assert from_mont(h) == [x[0], x[1], y[0], y[1]] and int(h[24]) == 0
    assert np.array_equal(bh, g2_row(R.g2_mul(R.G2_GEN, tau)))
    again = plk.OpeningKey.load(h, bh)
    h2, bh2 = again.points()
    assert np.array_equal(h, h2) and np.array_equal(bh, bh2)
    w = P.g1_mul(P.G1_GEN, 99)
    assert again.check(pair_words(P.g1_mul(w, tau), w))


def outside_subgroup():
    """An on-twist point not of order r: x = 1, 2, .. until x^3 + 4 (1 + u) is a square and r
    times the point is not the identity."""
    for k in range(1, 100):
        x = (k, 0)
        rhs = R.f2add(R.f2mul(R.f2mul(x, x), x), R.f2scale(R.XI, 4))
        y = R.f2sqrt(rhs) if R.f2_is_square(rhs) else None
        if y is None:
            continue
        q = (x, y)
        assert R.g2_is_on_curve(q)
        if R.g2_mul(q, r) is not None:
            return q
    raise AssertionError("no such point below x = 100")


def test_opening_key_load_refusals(plk):
    h, bh = plk.OpeningKey.setup(3).points()
    off = h.copy()
    off[12] ^= np.uint64(1)  # y.c0 leaves the twist
    big = h.copy()
    big[6:12] = P.int_to_limbs(P.P_MOD, 6)  # x.c1 = p: not canonical
    inf = np.zeros(25, dtype=np.uint64)
    inf[24] = 1
    stray = g2_row(outside_subgroup())
    for bad in (off, big, inf, stray):
        for args in ((bad, bh), (h, bad)):
            with pytest.raises(plk.PlonkError) as err:
                plk.OpeningKey.load(*args)
            assert err.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as err:
        plk.OpeningKey.setup(0)
    assert err.value.status == plk.PLK_E_ARG


def test_null_arguments(plk):
    lib = plk.plonk._lib()
    assert lib.plk_opening_key_setup(None, None) == plk.PLK_E_ARG
    assert lib.plk_pairing_check(None, None, None) == plk.PLK_E_ARG
    assert lib.plk_pairing_check_batch(None, None, None, 0, None) == plk.PLK_E_ARG
    assert lib.plk_debug_pairing(None, None, None, 0, None) == plk.PLK_E_ARG
    assert lib.plk_debug_f12_op(None, 0, None, None, 0, None) == plk.PLK_E_ARG
    assert lib.plk_debug_miller(None, None, None, None, None, 0, None) == plk.PLK_E_ARG
    from dusk_plonk_amd.prover import _bind
    b = _bind()
    assert b.plk_verifier_pairs(None, None, None, None, 0, None) == plk.PLK_E_ARG
    assert b.plk_verifier_verify(None, None, None, None, None, 0, None, None) == plk.PLK_E_ARG
    assert b.plk_verifier_verify_each(None, None, None, None, None, 0, None) == plk.PLK_E_ARG
