"""Operands and expected values for the per-operation tests of the pairing's tower
(csrc/pairing.hpp through plk_debug_f12_op / plk_debug_miller) — TEST INFRASTRUCTURE ONLY, shared
by tests/test_pairing_tower_cpu.py and tests/test_pairing_tower_gpu.py.

Values are big integers (tests/pairing_ref.py's representation: an Fp12 element is a list of six
(c0, c1) pairs); rows() / unrows() convert to and from the uint64[n, 72] rows of the entry points.
"""
from __future__ import annotations

import numpy as np

import pairing_ref as R
import pyref as P
from make_pairing_vectors import f12_from_row, f12_row
from test_field_gpu import edge_values, random_values

p = R.p
EDGES = edge_values(p, 381)
# the reduced set whose every pair is an Fp2 operand
CORE = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 380) % p, (1 << 352) - 1]

T3 = (0, 2)  # on y^2 = x^3 + 4, of order 3: outside the order-r subgroup, x = 0


def rows(elems) -> np.ndarray:
    return np.stack([f12_row(e) for e in elems])


def unrows(arr):
    return [f12_from_row(row) for row in arr]


def rand_fp(n, seed):
    return random_values(p, 381, n, seed)


def rand_f2(n, seed):
    v = rand_fp(2 * n, seed)
    return list(zip(v[0::2], v[1::2]))


def rand_f12(n, seed):
    v = rand_f2(6 * n, seed)
    return [v[6 * i: 6 * i + 6] for i in range(n)]


# --------------------------------------------------------------------------- Fp2 operands
def f2_operands():
    """Every pair of CORE; (a, a), (a, -a), (a, 0), (0, a) for every edge value a; (0, 0) and
    (p - 1, p - 1) (both among the pairs of CORE, asserted); random values."""
    out = [(a, b) for a in CORE for b in CORE]
    for a in EDGES:
        out += [(a, a), (a, -a % p), (a, 0), (0, a)]
    assert (0, 0) in out and (p - 1, p - 1) in out
    return out + rand_f2(40, 0xF2)


def f2_core():
    """The Fp2 values whose every ordered pair is an operand pair of f2_mul."""
    h = (p - 1) // 2
    return [(0, 0), (1, 0), (0, 1), (p - 1, 0), (0, p - 1), (p - 1, p - 1), (1, 1), (1, p - 1),
            (h, h), (h, h + 1), (h + 1, h + 1), ((1 << 380) % p, (1 << 352) - 1)] + rand_f2(2, 0xC0)


def pack_f2(vals):
    """Fp2 values six to a row (the last row padded with zeros) -> Fp12-shaped elements."""
    vals = list(vals) + [(0, 0)] * (-len(vals) % 6)
    return [vals[i: i + 6] for i in range(0, len(vals), 6)]


# --------------------------------------------------------------------------- Fp12 operands
def _unit(k, v=(1, 0)):
    return [v if i == k else (0, 0) for i in range(6)]


def line_shaped(seed):
    c0, c2 = rand_f2(2, seed)
    return R.line(c0, c2, rand_fp(1, seed + 1)[0])


def fp6_element(seed):
    v = rand_f2(3, seed)
    return [v[0], (0, 0), v[1], (0, 0), v[2], (0, 0)]


def f12_structured():
    """(name, element): the operands with structure the issue lists."""
    m1 = p - 1
    out = [("0", list(R.F12_ZERO)), ("1", list(R.F12_ONE)), ("-1", _unit(0, (m1, 0)))]
    out += [(f"w^{k}", _unit(k)) for k in range(1, 6)]
    for k in range(6):
        out += [(f"(p-1) w^{k}", _unit(k, (m1, 0))), (f"(p-1) u w^{k}", _unit(k, (0, m1)))]
    out += [("all p-1", [(m1, m1)] * 6),
            ("Fp2 subfield", _unit(0, rand_f2(1, 0x52)[0])),
            ("Fp6", fp6_element(0x56)),
            ("line", line_shaped(0x1E)),
            ("line c2 = 0", R.line(rand_f2(1, 0x1F)[0], (0, 0), 5))]
    return out


def f12_operands(n_random=8, seed=0x12):
    """The structured elements followed by random ones."""
    return [e for _, e in f12_structured()] + rand_f12(n_random, seed)


def line_operands():
    """(c0, c2, y) triples: y at every edge value next to random c0, c2; c2 == 0 (the line at a
    point with x = 0), c0 == 0, both, all zero, all p - 1; random ones."""
    c = rand_f2(2 * len(EDGES), 0x71)
    out = [(c[2 * i], c[2 * i + 1], y) for i, y in enumerate(EDGES)]
    a, b = rand_f2(2, 0x72)
    y = rand_fp(1, 0x73)[0]
    m1 = p - 1
    out += [(a, (0, 0), y), ((0, 0), b, y), ((0, 0), (0, 0), y), ((0, 0), (0, 0), 0), (a, b, 0),
            ((m1, m1), (m1, m1), m1), ((1, 0), (0, 0), 0)]
    return out + [(u, v, w) for u, v, w in zip(rand_f2(4, 0x74), rand_f2(4, 0x75), rand_fp(4, 0x76))]


def line_row(c0, c2, y) -> np.ndarray:
    """Row b of the mul_line op: c0 in limbs 0..11, c2 in 12..23, y in 24..29."""
    return f12_row([c0, c2, (y, 0), (0, 0), (0, 0), (0, 0)])


_CYC = {}


def cyclotomic(n, seed=0xC7):
    """n elements of the cyclotomic subgroup: g, g^2, g^3, .. for g = easy_part(random), then the
    conjugate of the last one in place of it (n > 1)."""
    if (n, seed) not in _CYC:
        g = R.easy_part(rand_f12(1, seed)[0])
        out = [g]
        while len(out) < n:
            out.append(R.f12mul(out[-1], g))
        if n > 1:
            out[-1] = R.f12conj(out[-1])
        _CYC[(n, seed)] = out
    return [list(e) for e in _CYC[(n, seed)]]


# --------------------------------------------------------------------------- expected values
_MEMO = {}


def expected(op, a, b=None):
    """The restatement's value of one op on big-integer operands (memoised: the Frobenius powers
    cost ~0.1 s each). b: an element, or the (c0, c2, y) triple of mul_line."""
    key = (op, repr(a), repr(b))
    if key not in _MEMO:
        _MEMO[key] = _expected(op, a, b)
    return _MEMO[key]


def _expected(op, a, b):
    if op == "f2_mul":
        return [R.f2mul(x, y) for x, y in zip(a, b)]
    if op == "f2_sqr":
        return [R.f2mul(x, x) for x in a]
    if op == "f2_inv":
        return [R.f2inv(x) for x in a]  # pow(0, p - 2) = 0: the inverse of zero is zero
    if op == "f2_mul_xi":
        return [R.f2mul(x, R.XI) for x in a]
    if op == "mul":
        return R.f12mul(a, b)
    if op in ("sqr", "cyc_sqr"):
        return R.f12sqr(a)
    if op == "conj":
        return R.f12conj(a)
    if op == "frob1":
        return R.f12frob(a, 1)
    if op == "frob2":
        return R.f12frob(a, 2)
    if op == "mul_line":
        return R.f12mul(a, R.line(*b))
    if op == "inv_even":
        return R.f12inv([x if i % 2 == 0 else (0, 0) for i, x in enumerate(a)])
    raise ValueError(op)


# --------------------------------------------------------------------------- G1 / G2 for Miller
def g1_rows(pts) -> np.ndarray:
    return P.g1_vec_to_np(list(pts))


def miller_pair(p0, q0, p1, q1):
    """What plk_debug_miller's two-pair form returns: ML(p0, q0) ML(-p1, q1)."""
    return R.f12mul(R.miller_loop(p0, q0), R.miller_loop(P.g1_neg(p1), q1))


def off_subgroup_pairs(tau, w):
    """(name, (C, W)) pairs of a pairing check with the order-3 point T = (0, 2) in them, next to
    the honest pair (tau w, w): what plk_pairing_check[_batch] answers for on-curve points outside
    G1 is pinned against the restatement on these."""
    c = P.g1_mul(w, tau)
    wt = P.g1_add(w, T3)
    return [("(T, T)", (T3, T3)), ("(C + T, W)", (P.g1_add(c, T3), w)), ("(C, W + T)", (c, wt)),
            ("(T, O)", (T3, None)), ("(tau (W + T), W + T)", (P.g1_mul(wt, tau), wt))]
