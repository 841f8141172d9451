"""Reference of the closed-form top of the quotient (csrc/quotient_top.hpp): the whole numerator
N of round 3 as a polynomial, by pure-Python big-integer polynomial arithmetic, and t = N / Z_H.

Poly carries a coefficient list modulo r and the operators + - * with polynomials and integers
(and % r as a no-op), so the gate definitions of tests/prover_stage_ref.py (delta, logic_widget,
fixed_base_widget, var_base_widget: written for a row's VALUES) evaluate unchanged on the
polynomials themselves. Products are schoolbook (mul_schoolbook, O(n^2)) or, for the large sizes,
one big-integer product of the Kronecker-packed coefficients (mul_kronecker: exact, every slot
holds the unreduced sum of at most 2^16 products below 2^510); test_quotient_top_cpu.py holds
the two against each other. Nothing here is the code under test."""
from __future__ import annotations

import prover_stage_ref as S

r = S.r
SLOT = 66  # bytes per Kronecker slot: 528 bits > 2 * 255 + 16


def mul_schoolbook(a, b):
    if not a or not b:
        return []
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return [v % r for v in out]


def mul_kronecker(a, b):
    if not a or not b:
        return []
    assert min(len(a), len(b)) < 1 << 16
    pa = int.from_bytes(b"".join(x.to_bytes(SLOT, "little") for x in a), "little")
    pb = int.from_bytes(b"".join(x.to_bytes(SLOT, "little") for x in b), "little")
    cnt = len(a) + len(b) - 1
    raw = (pa * pb).to_bytes(SLOT * (cnt + 1), "little")
    return [int.from_bytes(raw[SLOT * i:SLOT * (i + 1)], "little") % r for i in range(cnt)]


class Poly:
    def __init__(self, c, mul=mul_schoolbook):
        self.c = [x % r for x in c]
        self.mul = mul

    def _lift(self, o):
        return o if isinstance(o, Poly) else Poly([o], self.mul)

    def __add__(self, o):
        o = self._lift(o)
        m = max(len(self.c), len(o.c))
        a, b = self.c + [0] * (m - len(self.c)), o.c + [0] * (m - len(o.c))
        return Poly([x + y for x, y in zip(a, b)], self.mul)

    __radd__ = __add__

    def __neg__(self):
        return Poly([-x for x in self.c], self.mul)

    def __sub__(self, o):
        return self + (-self._lift(o))

    def __rsub__(self, o):
        return self._lift(o) - self

    def __mul__(self, o):
        if isinstance(o, Poly):
            return Poly(self.mul(self.c, o.c), self.mul)
        return Poly([x * o for x in self.c], self.mul)

    __rmul__ = __mul__

    def __mod__(self, _):
        return self

    def rot(self, w):
        """p(w X)"""
        out, s = [], 1
        for x in self.c:
            out.append(x * s)
            s = s * w % r
        return Poly(out, self.mul)


def numerator(n, omega, wires, z, sel, sigma, pis, ch, flags, mul=mul_schoolbook):
    """N(X) as a coefficient list of length 5n + 7. wires: 4 lists (n + 2 coefficients), z (n + 3),
    sel: 11 lists in S.SEL order and sigma: 4 lists (n each), pis: [(gate index, value)], ch: dict as
    in prover_stage_ref.quotient, flags: 1 range | 2 logic | 4 fixed | 8 var."""
    P = lambda c: Poly(c, mul)  # noqa: E731
    a, b, c, d = (P(w) for w in wires)
    an, bn, dn = a.rot(omega), b.rot(omega), d.rot(omega)
    zp = P(z)
    zn = zp.rot(omega)
    q = [P(s) for s in sel]
    n_inv = pow(n, -1, r)
    l1 = P([n_inv] * n)
    pi = P([0])
    for idx, v in pis:  # L_idx(X) = L_0(w^-idx X)
        pi = pi + v * l1.rot(pow(omega, -idx, r))
    al, be, ga = ch["alpha"], ch["beta"], ch["gamma"]
    t = q[S.QARITH] * (q[S.QM] * a * b + q[S.QL] * a + q[S.QR] * b + q[S.QO] * c + q[S.Q4] * d + q[S.QC]) + pi
    if flags & 1:
        k = ch["range_sep"] ** 2 % r
        t = t + q[S.QRANGE] * ch["range_sep"] * (S.delta(c - 4 * d) + S.delta(b - 4 * c) * k
                                                 + S.delta(a - 4 * b) * (k ** 2 % r)
                                                 + S.delta(dn - 4 * a) * (k ** 3 % r))
    x = P([0, 1])
    ident, copy = zp, zn
    for w, kk, sg in zip((a, b, c, d), (1, 7, 13, 17), sigma):
        ident = ident * (w + be * kk * x + ga)
        copy = copy * (w + be * P(sg) + ga)
    t = t + al * (ident - copy) + al * al % r * ((zp - 1) * l1)
    row = (a, an, b, bn, c, d, dn)
    if flags & 2:
        t = t + q[S.QLOGIC] * ch["logic_sep"] * S.logic_widget(*row, q[S.QC], ch["logic_sep"] ** 2 % r)
    if flags & 4:
        t = t + q[S.QFIXED] * ch["fixed_sep"] * S.fixed_base_widget(*row, q[S.QL], q[S.QR], q[S.QC],
                                                                    ch["fixed_sep"] ** 2 % r)
    if flags & 8:
        t = t + q[S.QVAR] * ch["var_sep"] * S.var_base_widget(*row, ch["var_sep"] ** 2 % r)
    out = t.c + [0] * (5 * n + 7 - len(t.c))
    assert len(out) == 5 * n + 7 or not any(out[5 * n + 7:]), "deg N <= 5n + 6"
    return out[:5 * n + 7]


def divide_by_zh(num, n):
    """(t, remainder is zero) with num = t (X^n - 1): t[k] = t[k - n] - num[k]."""
    t = []
    for k in range(len(num) - n):
        t.append(((t[k - n] if k >= n else 0) - num[k]) % r)
    exact = all((t[k - n] if k - n < len(t) else 0) == num[k] % r for k in range(len(num) - n, len(num)))
    return t, exact
