"""BLS12-381 optimal ate pairing on Python big integers — TEST INFRASTRUCTURE ONLY.

Written from the mathematics, independently of csrc/pairing.hpp: affine G2 arithmetic, a Miller
loop whose lines are multiplied in as full Fp12 elements, and the plain final power
(p^12 - 1) / r by square-and-multiply. G1 comes from oracle/pyref.py.

Representation: Fp2 = Fp[u] / (u^2 + 1) as (c0, c1); Fp12 = Fp2[w] / (w^6 - xi), xi = 1 + u, as
the six Fp2 coefficients of w^0 .. w^5. The twist E': y^2 = x^3 + 4 xi is of M type: (x, y) on
E' maps to (x / w^2, y / w^3) on E over Fp12, so the line through T with slope lam, evaluated at
P = (xP, yP) in G1 and scaled by w^3 (a factor of Fp4, killed by the final power), is
    (lam xT - yT) + (-lam xP) w^2 + yP w^3.
The loop parameter x = -0xd201000000010000 is negative: the loop runs over |x| and the result is
conjugated.
"""
from __future__ import annotations

import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import pyref as P  # noqa: E402

p = P.P_MOD
r = P.R_MOD
X_ABS = 0xD201000000010000
XI = (1, 1)
FINAL_POWER = (p ** 12 - 1) // r
assert (p ** 12 - 1) % r == 0

# the standard G2 generator (zkcrypto bls12_381 G2Affine::generator)
G2_GEN = (
    (int("024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d177"
         "0bac0326a805bbefd48056c8c121bdb8", 16),
     int("13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049"
         "334cf11213945d57e5ac7d055d042b7e", 16)),
    (int("0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c"
         "923ac9cc3baca289e193548608b82801", 16),
     int("0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab"
         "3f370d275cec1da1aaa9075ff05f79be", 16)),
)


# --------------------------------------------------------------------------- Fp2
def f2add(a, b):
    return ((a[0] + b[0]) % p, (a[1] + b[1]) % p)


def f2sub(a, b):
    return ((a[0] - b[0]) % p, (a[1] - b[1]) % p)


def f2neg(a):
    return (-a[0] % p, -a[1] % p)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def f2scale(a, k):
    return (a[0] * k % p, a[1] * k % p)


def f2inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], p - 2, p)
    return (a[0] * d % p, -a[1] * d % p)


def f2pow(a, e):
    out = (1, 0)
    for bit in bin(e)[2:]:
        out = f2mul(out, out)
        if bit == "1":
            out = f2mul(out, a)
    return out


def f2_is_square(a):
    """Euler's criterion in Fp2 through the norm to Fp."""
    n = (a[0] * a[0] + a[1] * a[1]) % p
    return n == 0 or pow(n, (p - 1) // 2, p) == 1


def f2sqrt(a):
    """A square root in Fp2 (p = 3 mod 4; Adj and Rodriguez-Henriquez, algorithm 9), or None."""
    if a == (0, 0):
        return (0, 0)
    a1 = f2pow(a, (p - 3) // 4)
    alpha = f2mul(f2mul(a1, a1), a)
    x0 = f2mul(a1, a)
    if alpha == (p - 1, 0):
        cand = f2mul((0, 1), x0)
    else:
        b = f2pow(f2add((1, 0), alpha), (p - 1) // 2)
        cand = f2mul(b, x0)
    return cand if f2mul(cand, cand) == (a[0] % p, a[1] % p) else None


# --------------------------------------------------------------------------- Fp12
F12_ONE = [(1, 0)] + [(0, 0)] * 5


def f12mul(a, b):
    c = [(0, 0)] * 11
    for i in range(6):
        for j in range(6):
            c[i + j] = f2add(c[i + j], f2mul(a[i], b[j]))
    return [f2add(c[k], f2mul(XI, c[k + 6])) if k < 5 else c[k] for k in range(6)]


def f12pow(a, e):
    out = list(F12_ONE)
    for bit in bin(e)[2:] if e else "":
        out = f12mul(out, out)
        if bit == "1":
            out = f12mul(out, a)
    return out


def f12conj(a):
    """a^(p^6): w -> -w."""
    return [a[i] if i % 2 == 0 else f2neg(a[i]) for i in range(6)]


# What the per-operation tests of csrc/pairing.hpp compare with (tests/pairing_tower_ops.py). Each
# is derived another way than the product's formula: the square is the general product, a
# Frobenius map a literal power, the inverse a polynomial gcd.
F12_ZERO = [(0, 0)] * 6


def f12sqr(a):
    return f12mul(a, a)


def f12frob(a, k):
    """a^(p^k) as a literal power (no coefficient table)."""
    return f12pow(a, p ** k)


def _poly_trim(a):
    while a and a[-1] == (0, 0):
        a = a[:-1]
    return a


def _poly_divmod(a, b):
    """Quotient and remainder in Fp2[w]; coefficient lists, lowest first, b trimmed and not zero."""
    a, q = list(a), [(0, 0)] * max(len(a) - len(b) + 1, 0)
    lead = f2inv(b[-1])
    for k in range(len(a) - len(b), -1, -1):
        c = f2mul(a[k + len(b) - 1], lead)
        q[k] = c
        for i, bi in enumerate(b):
            a[k + i] = f2sub(a[k + i], f2mul(c, bi))
    return q, _poly_trim(a[:len(b) - 1])


def _poly_mul(a, b):
    out = [(0, 0)] * (len(a) + len(b) - 1) if a and b else []
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            out[i + j] = f2add(out[i + j], f2mul(ai, bj))
    return out


def _poly_sub(a, b):
    n = max(len(a), len(b))
    a, b = a + [(0, 0)] * (n - len(a)), b + [(0, 0)] * (n - len(b))
    return _poly_trim([f2sub(x, y) for x, y in zip(a, b)])


def f12inv(a):
    """1 / a by the extended Euclidean algorithm on a(w) and w^6 - xi in Fp2[w] (w^6 - xi is
    irreducible, so the gcd of a non-zero a is a constant). The inverse of zero is zero, the
    product's convention."""
    r0, r1 = [f2neg(XI)] + [(0, 0)] * 5 + [(1, 0)], _poly_trim(list(a))
    t0, t1 = [], [(1, 0)]  # r_i = t_i a mod (w^6 - xi)
    if not r1:
        return list(F12_ZERO)
    while len(r1) > 1:
        q, rem = _poly_divmod(r0, r1)
        r0, r1, t0, t1 = r1, rem, t1, _poly_sub(t0, _poly_mul(q, t1))
    c = f2inv(r1[0])
    out = [f2mul(c, x) for x in t1]
    assert len(out) <= 6
    return out + [(0, 0)] * (6 - len(out))


def easy_part(f):
    """f^((p^6 - 1)(p^2 + 1)): an element of the cyclotomic subgroup (order p^4 - p^2 + 1)."""
    g = f12mul(f12conj(f), f12inv(f))
    return f12mul(f12frob(g, 2), g)


def line(c0, c2, y):
    """The Fp12 element c0 + c2 w^2 + y w^3 (y in Fp) of a Miller line."""
    return [c0, (0, 0), c2, (y % p, 0), (0, 0), (0, 0)]


# --------------------------------------------------------------------------- G2 (affine)
def g2_is_on_curve(q) -> bool:
    if q is None:
        return True
    x, y = q
    return f2mul(y, y) == f2add(f2mul(f2mul(x, x), x), f2scale(XI, 4))


def g2_neg(q):
    return None if q is None else (q[0], f2neg(q[1]))


def _g2_step(t, q):
    """(t + q, slope) for finite t, q with t != -q."""
    if t == q:
        lam = f2mul(f2scale(f2mul(t[0], t[0]), 3), f2inv(f2scale(t[1], 2)))
    else:
        lam = f2mul(f2sub(q[1], t[1]), f2inv(f2sub(q[0], t[0])))
    x3 = f2sub(f2sub(f2mul(lam, lam), t[0]), q[0])
    y3 = f2sub(f2mul(lam, f2sub(t[0], x3)), t[1])
    return (x3, y3), lam


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0] and a[1] != b[1]:
        return None
    if a == b and a[1] == (0, 0):
        return None
    return _g2_step(a, b)[0]


def g2_mul(q, s: int):
    acc = None
    for bit in bin(s)[2:] if s else "":
        acc = g2_add(acc, acc)
        if bit == "1":
            acc = g2_add(acc, q)
    return acc


# --------------------------------------------------------------------------- the pairing
def miller_loop(pt, q):
    """f_{|x|, Q}(P), conjugated (x < 0). An infinite operand gives one."""
    if pt is None or q is None:
        return list(F12_ONE)
    xp, yp = pt
    f = list(F12_ONE)
    t = q
    for bit in bin(X_ABS)[3:]:
        f = f12mul(f, f)
        for other in ([t] if bit == "0" else [t, q]):
            t_new, lam = _g2_step(t, other)
            line = [f2sub(f2mul(lam, t[0]), t[1]), (0, 0), f2scale(f2neg(lam), xp), (yp, 0),
                    (0, 0), (0, 0)]
            f = f12mul(f, line)
            t = t_new
    return f12conj(f)


def final_power(f):
    return f12pow(f, FINAL_POWER)


def final_power_cubed(f):
    """f^(3 (p^12 - 1) / r): what the product's f12_final_exp computes."""
    return f12pow(final_power(f), 3)


def pairing(pt, q):
    """e(P, Q) in the order-r subgroup of Fp12*."""
    return final_power(miller_loop(pt, q))


def pairing_cubed(pt, q):
    """e(P, Q)^3: what the product's addition chain computes (plk_debug_pairing)."""
    e = pairing(pt, q)
    return f12mul(f12mul(e, e), e)


def pairing_check(c, w, h, beta_h) -> bool:
    """e(c, H) == e(w, beta_h)."""
    f = f12mul(miller_loop(c, h), miller_loop(P.g1_neg(w), beta_h))
    return final_power(f) == F12_ONE
