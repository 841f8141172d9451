"""The closed-form top of the quotient on the host (csrc/quotient_top.hpp through stage
"quotient_top" of plk_debug_prover_stage, no GPU): t[4n .. 4n + 6] = N[5n .. 5n + 6] from seven
coefficients per factor polynomial, against the FULL numerator N formed by schoolbook
multiplication in Python integers (tests/quotient_top_ref.py). Exact equality, no tolerance.

n = 16 is the smallest size on the four-block path: the seven-coefficient slice of a selector
(degree n - 1) reaches down to coefficient 9 and of a constant to degree -6, which exercises the
alignment of sums; n = 64 has every slice far above the constants. Every combination of the four
has_* flags runs at both sizes."""
from __future__ import annotations

import random

import pytest

import prover_stage_ref as S
import quotient_top_ref as Q

r = S.r
NAMES = ("alpha", "beta", "gamma", "range_sep", "logic_sep", "fixed_sep", "var_sep")


def omega_of(n):
    w = pow(7, (r - 1) // n, r)
    assert pow(w, n, r) == 1 and pow(w, n // 2, r) == r - 1
    return w


def blind(rng, n, count, zero_blinders=False):
    """A random polynomial of degree < n plus b(X)(X^n - 1), b of `count` coefficients."""
    p = [rng.randrange(r) for _ in range(n)] + [0] * count
    for i in range(count):
        b = 0 if zero_blinders else rng.randrange(1, r)
        p[i] = (p[i] - b) % r
        p[n + i] = b
    return p


def case(n, seed, edge=None):
    rng = random.Random(seed)
    c = {"wires": [blind(rng, n, 2, edge == "zero_blinders") for _ in range(4)],
         "z": blind(rng, n, 3, edge == "zero_blinders"),
         "sel": [[rng.randrange(r) for _ in range(n)] for _ in range(11)],
         "sigma": [[rng.randrange(r) for _ in range(n)] for _ in range(4)],
         "pis": [(rng.randrange(n), rng.randrange(r)) for _ in range(3)],
         "ch": {k: rng.randrange(r) for k in NAMES}}
    if edge == "top_minus_one":  # every top coefficient of every wire and of z is r - 1
        for w in c["wires"]:
            w[n - 5:] = [r - 1] * 7
        c["z"][n - 4:] = [r - 1] * 7
    if edge == "zero_selector_top":  # q_m and q_range end in seven zero coefficients
        for s in (S.QM, S.QRANGE):
            c["sel"][s][n - 7:] = [0] * 7
    if edge == "pi_first_last":
        c["pis"] = [(0, rng.randrange(1, r)), (n - 1, rng.randrange(1, r))]
    if edge == "no_pi":
        c["pis"] = []
    return c


def stage_q(plk, n, omega, c, flags):
    top = lambda p, hi: S.words_np(p[hi - 6:hi + 1])  # noqa: E731  coefficients hi-6 .. hi
    arrays = [
        [top(w, n + 1) for w in c["wires"]], top(c["z"], n + 2), [top(s, n - 1) for s in c["sel"]],
        [top(s, n - 1) for s in c["sigma"]], S.words_np([pow(n, -1, r)] * 7)]
    import numpy as np
    arrays = [np.concatenate(a) if isinstance(a, list) else a for a in arrays]
    scalars = S.words_np([c["ch"][k] for k in NAMES] + [omega] + [v for _, v in c["pis"]])
    params = [n.bit_length() - 1, flags] + [i for i, _ in c["pis"]]
    return [S.unword(w) for w in S.from_np(plk.plonk.quotient_top(arrays, scalars, params))]


def reference_q(n, omega, c, flags):
    num = Q.numerator(n, omega, c["wires"], c["z"], c["sel"], c["sigma"], c["pis"], c["ch"], flags,
                      mul=Q.mul_schoolbook)
    assert len(num) == 5 * n + 7
    return num[5 * n:]


@pytest.mark.parametrize("n", [16, 64])
def test_q_equals_full_product_every_flag_set(plk, n):
    omega = omega_of(n)
    for flags in range(16):
        c = case(n, 100 * n + flags)
        assert stage_q(plk, n, omega, c, flags) == reference_q(n, omega, c, flags), flags


@pytest.mark.parametrize("edge", ["zero_blinders", "top_minus_one", "zero_selector_top",
                                  "pi_first_last", "no_pi"])
@pytest.mark.parametrize("n", [16, 64])
def test_q_edge_operands(plk, n, edge):
    omega = omega_of(n)
    for flags in (0, 15):
        c = case(n, 7 * n + flags, edge)
        want = reference_q(n, omega, c, flags)
        assert stage_q(plk, n, omega, c, flags) == want, flags
        if edge == "zero_blinders":  # the degree bound is not the degree: the top of N is zero
            assert want == [0] * 7


def test_kronecker_product_equals_schoolbook():
    rng = random.Random(5)
    for la, lb in ((1, 1), (7, 3), (40, 66), (130, 17)):
        a = [rng.choice((0, 1, r - 1, rng.randrange(r))) for _ in range(la)]
        b = [rng.choice((0, 1, r - 1, rng.randrange(r))) for _ in range(lb)]
        assert Q.mul_kronecker(a, b) == Q.mul_schoolbook(a, b)
    assert Q.mul_kronecker([r - 1] * 50, [r - 1] * 50) == Q.mul_schoolbook([r - 1] * 50, [r - 1] * 50)


def test_division_by_zh_is_exact_only_for_multiples():
    rng = random.Random(6)
    n = 16
    t = [rng.randrange(r) for _ in range(4 * n + 7)]
    num = Q.mul_schoolbook(t, [r - 1] + [0] * (n - 1) + [1])
    got, exact = Q.divide_by_zh(num, n)
    assert exact and got == t
    num[3] = (num[3] + 1) % r
    assert not Q.divide_by_zh(num, n)[1]


def test_stage_refuses_bad_shapes(plk):
    c = case(16, 1)
    omega = omega_of(16)
    good = stage_q(plk, 16, omega, c, 0)
    assert len(good) == 7
    c["pis"] = [(16, 5)]  # a gate index outside the domain
    with pytest.raises(plk.PlonkError):
        stage_q(plk, 16, omega, c, 0)
    with pytest.raises(plk.PlonkError):
        stage_q(plk, 8, omega_of(8), case(8, 1), 0)  # n = 8 is not on this path
