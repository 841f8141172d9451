"""Plain reference of the prover's round kernels (csrc/prover_kernels.hip), in two parts.

Values: one function per stage computing the stage's definition modulo r in Python integers on
plain (decoded) field values: the quotient's row formula from the gate definitions (arithmetic,
PI, range, permutation with K = 7, 13, 17, (z - 1) L1 alpha^2, logic, fixed-base and variable-base
widgets, times 1 / v_h of the block, the next row taken inside the block), the permutation's
numerators and denominators, prefix / suffix scans, Horner evaluation, the linear combination, the
power scaling and synthetic division (pyref.ruffini).

Bounds: a limb-exact model of the redundant-form chains of k_quotient<FINAL>, k_perm_numden,
k_coset_combine, k_pi_sparse, k_lincomb and k_eval_partial on the 9 x 29-bit limbs of rx_ref.FR.
Each chain is written ONCE over an algebra object and run by two of them: Concrete carries exact
limb rows (products are the one exact Montgomery value, rx_ref.RxField.mont), Bounds carries the
(largest lower limb, largest top limb, largest value) of every intermediate from the input
contract alone. Both assert what the device code relies on at every step: a 64-bit column
accumulator of the unsplit rx_mul / rx_mul_add never reaches 2^64, no limb of a carry-free sum or
difference leaves 32 bits or goes negative, every product's value stays inside the bound that
keeps its result below 2r, and each consumer's precondition of ffr.hpp holds (rx_add / rx_sub /
rx_is_zero / rx_pack_canonical: normalised operands below 2r).

The input contract is canonical words below r: the transforms' stores (ntt.hip) and every other
producer of these arrays end in rx_pack_canonical or a packed fe_* operation."""
from __future__ import annotations

import random

import pyref as P
import rx_ref as R

F = R.FR
r = F.p
L, B, MASK = F.L, F.B, F.mask
U32, U64 = 1 << 32, 1 << 64
TOP_SHIFT = B * (L - 1)
MONT = P.FR_R % r            # R = 2^256 mod r
SH5 = 32                     # R' / R = 2^5
INV32 = pow(32, -1, r)

SEL = ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith", "q_range", "q_logic", "q_fixed", "q_var")
QM, QL, QR, QO, Q4, QC, QARITH, QRANGE, QLOGIC, QFIXED, QVAR = range(11)
EDWARDS_D = (-10240 * pow(10241, -1, r)) % r


def word(x: int, e: int = 0) -> int:
    """The stored word of the value x at exponent e (QuotientArgs): x R 2^(-5e) mod r."""
    return x * MONT * pow(32, -e, r) % r


def unword(w: int) -> int:
    return w * P.FR_RINV % r


# =============================================================================== values
def delta(f: int) -> int:
    return f * (f - 1) * (f - 2) * (f - 3) % r


def logic_widget(a, a_n, b, b_n, c, d, d_n, q_c, k) -> int:
    """dusk-plonk logic gate on the quads a' = a_next - 4a, b', d' and w = c."""
    qa, qb, qd, w = (a_n - 4 * a) % r, (b_n - 4 * b) % r, (d_n - 4 * d) % r, c
    s = qa + qb
    f = w * (w * (4 * w - 18 * s + 81) + 18 * (qa * qa + qb * qb) - 81 * s + 83)
    xor_and = 3 * (s + qd) - 2 * f + q_c * (9 * qd - 3 * s)
    return (delta(qa) + delta(qb) * k + delta(qd) * k ** 2 + (w - qa * qb) * k ** 3 + xor_and * k ** 4) % r


def fixed_base_widget(a, a_n, b, b_n, c, d, d_n, q_l, q_r, q_c, k) -> int:
    """Fixed-base scalar multiplication gate: (a, b) the point accumulator, d the scalar
    accumulator, c = xy_alpha, (q_l, q_r, q_c) = (x_beta, y_beta, x_beta y_beta)."""
    bit = (d_n - 2 * d) % r
    y_alpha = (bit * bit * (q_r - 1) + 1) % r
    x_alpha = q_l * bit % r
    prod = c * a * b * EDWARDS_D % r
    x_check = a_n * (1 + prod) - (a * y_alpha + b * x_alpha)
    y_check = b_n * (1 - prod) - (b * y_alpha + a * x_alpha)
    return (bit * (bit - 1) * (bit + 1) + (bit * q_c - c) * k + x_check * k ** 2 + y_check * k ** 3) % r


def var_base_widget(a, a_n, b, b_n, c, d, d_n, k) -> int:
    """Curve addition gate (x1, y1, x2, y2) = (a, b, c, d), next row (x3, y3, ., x1 y2)."""
    x1, y1, x2, y2, x3, y3, x1y2 = a, b, c, d, a_n, b_n, d_n
    dp = EDWARDS_D * x1y2 * y1 * x2 % r
    return ((x1 * y2 - x1y2) + (x1y2 + y1 * x2 - x3 * (1 + dp)) * k
            + (y1 * y2 + x1 * x2 - y3 * (1 - dp)) * k ** 2) % r


def quotient(n, blocks, a, b, c, d, z, pi, l1, sel, sigma, elements, ch, s_m, vh_inv, flags):
    """t over blocks * n points (plain values in and out). pi None: no public inputs. sel: 11 rows,
    sigma: 4 rows. ch: dict alpha beta gamma range_sep logic_sep fixed_sep var_sep. flags: dict
    range logic fixed var (a widget whose flag is off contributes nothing, whatever its selector)."""
    al, be, ga = ch["alpha"], ch["beta"], ch["gamma"]
    out = []
    for i in range(blocks * n):
        m, u = divmod(i, n)
        nx = m * n + (u + 1) % n
        x = s_m[m] * elements[u] % r
        q = [row[i] for row in sel]
        t = q[QARITH] * (q[QM] * a[i] * b[i] + q[QL] * a[i] + q[QR] * b[i] + q[QO] * c[i] + q[Q4] * d[i] + q[QC])
        if pi is not None:
            t += pi[i]
        if flags["range"]:
            k = ch["range_sep"] ** 2 % r
            t += q[QRANGE] * ch["range_sep"] * (delta((c[i] - 4 * d[i]) % r) + delta((b[i] - 4 * c[i]) % r) * k
                                                + delta((a[i] - 4 * b[i]) % r) * k ** 2
                                                + delta((d[nx] - 4 * a[i]) % r) * k ** 3)
        ident = z[i]
        copy = z[nx]
        for w, kk, sg in zip((a, b, c, d), (1, 7, 13, 17), sigma):
            ident = ident * (w[i] + be * kk * x + ga) % r
            copy = copy * (w[i] + be * sg[i] + ga) % r
        t += al * (ident - copy) + al * al * (z[i] - 1) * l1[i]
        nxt = (a[i], a[nx], b[i], b[nx], c[i], d[i], d[nx])
        if flags["logic"]:
            t += q[QLOGIC] * ch["logic_sep"] * logic_widget(*nxt, q[QC], ch["logic_sep"] ** 2 % r)
        if flags["fixed"]:
            t += q[QFIXED] * ch["fixed_sep"] * fixed_base_widget(*nxt, q[QL], q[QR], q[QC], ch["fixed_sep"] ** 2 % r)
        if flags["var"]:
            t += q[QVAR] * ch["var_sep"] * var_base_widget(*nxt, ch["var_sep"] ** 2 % r)
        out.append(t * vh_inv[m] % r)
    return out


def perm_numden(n, wires, sigmas, elements, beta, gamma, ks=(1, 7, 13, 17)):
    """wires, sigmas: 4 lists of n. Returns (num, den)."""
    num, den = [], []
    for i in range(n):
        nu = de = 1
        for col in range(4):
            nu = nu * (wires[col][i] + beta * ks[col] * elements[i] + gamma) % r
            de = de * (wires[col][i] + beta * sigmas[col][i] + gamma) % r
        num.append(nu)
        den.append(de)
    return num, den


def scan(vals, mul: bool, suffix: bool, exclusive: bool):
    """(outputs, grand total): prefix (suffix: from the top) products or sums."""
    seq = list(reversed(vals)) if suffix else list(vals)
    out, run = [], 1 if mul else 0
    for v in seq:
        nxt = run * v % r if mul else (run + v) % r
        out.append(run if exclusive else nxt)
        run = nxt
    return (list(reversed(out)) if suffix else out), run


def pi_sparse(n, blocks, l1, idx, vals):
    return [sum(v * l1[m * n + (u - i) % n] for i, v in zip(idx, vals)) % r
            for m in range(blocks) for u in range(n)]


def pi_coef(k, idx, vals):
    """The coefficients of the polynomial with value vals[j] at w^idx[j] and 0 elsewhere on H_n."""
    n = 1 << k
    w_inv = pow(P.omega(k), -1, r)
    n_inv = pow(n, -1, r)
    return [sum(v * pow(w_inv, i * j % n, r) for i, v in zip(idx, vals)) * n_inv % r for j in range(n)]


def coset_combine(n, blocks, vals, mat):
    """out[l n + k] = sum_m mat[l][m] vals[m n + k]."""
    return [sum(mat[l][m] * vals[m * n + k] for m in range(blocks)) % r
            for l in range(blocks) for k in range(n)]


def lincomb(polys, scalars, len_out):
    return [sum(s * p[j] for s, p in zip(scalars, polys) if j < len(p)) % r for j in range(len_out)]


def scale_powers(c, x, shift):
    out, pw = [], pow(x, shift, r)
    for v in c:
        out.append(v * pw % r)
        pw = pw * x % r
    return out


# ================================================================================ bounds
def borrow_free(c: int) -> tuple:
    """ffr.hpp rx_multiple(c, true): c r with every limb below the top raised by 2^B - 1 (2^B for
    limb 0), borrowed from the limb above."""
    m = list(F.limbs(c * r))
    m[0] += 1 << B
    for i in range(1, L - 1):
        m[i] += (1 << B) - 1
    m[L - 1] -= 1
    assert F.value(m) == c * r
    return tuple(m)


class Concrete:
    """Exact limb rows. A word argument is the packed canonical word in memory."""

    def __init__(self):
        self.max_column = 0
        self.max_limb = 0

    def _u32(self, row, what):
        assert min(row) >= 0 and max(row) < U32, f"{what}: a limb of {row} leaves 32 bits"
        self.max_limb = max(self.max_limb, max(row))
        return tuple(row)

    def ld(self, w):
        assert 0 <= w < r, "input contract: canonical words"
        return F.limbs(w)

    def unpack(self, w):  # an LDS value left by pack: below 2^256
        assert 0 <= w < 1 << 256
        return F.limbs(w)

    def const(self, v):
        return F.limbs(v)

    def _norm2r(self, a, what):
        assert F.normalised(a) and F.value(a) < 2 * r, f"{what}: operand not normalised below 2r: {a}"

    def _prod(self, pairs, what):
        n = 0
        for x, y in pairs:
            self._u32(x, what), self._u32(y, what)
            n += F.value(x) * F.value(y)
        (a, b), (c, d) = pairs[0], pairs[1] if len(pairs) > 1 else ((0,) * L, (0,) * L)
        col = R.unsplit_mul_add_max_column(F, a, b, c, d)
        assert col < U64, f"{what}: column accumulator {col} reaches 2^64"
        self.max_column = max(self.max_column, col)
        assert n < F.prod_bound, f"{what}: product value outside the bound that keeps the result below 2r"
        t = F.mont(n)
        assert t < 2 * r
        return F.limbs(t)

    def mul(self, a, b, what="rx_mul"):
        return self._prod([(a, b)], what)

    def mul_add(self, a, b, c, d, what="rx_mul_add"):
        return self._prod([(a, b), (c, d)], what)

    def add(self, a, b, what="rx_add"):
        self._norm2r(a, what), self._norm2r(b, what)
        s = F.value(a) + F.value(b)
        return F.limbs(s - 2 * r if s >= 2 * r else s)

    def sub(self, a, b, what="rx_sub"):
        self._norm2r(a, what), self._norm2r(b, what)
        s = F.value(a) - F.value(b)
        return F.limbs(s + 2 * r if s < 0 else s)

    def sum_u(self, *rows, what="carry-free sum"):
        return self._u32([sum(c) for c in zip(*rows)], what)

    def norm(self, a, what="rx_norm"):
        out, c = [], 0
        for i, v in enumerate(a):
            t = v + c
            assert t < U32, what
            out.append(t if i == L - 1 else t & MASK)
            c = t >> B
        assert F.value(out) == F.value(a)
        return tuple(out)

    def sub_u(self, a, b, cp, what="rx_sub_u"):
        q = borrow_free(cp)
        t = self._u32([x + m for x, m in zip(a, q)], what)
        return self._u32([x - y for x, y in zip(t, b)], f"{what}<{cp}>")

    def is_zero(self, a, what="rx_is_zero"):
        self._norm2r(a, what)
        return F.value(a) in (0, r)

    def pack(self, a, what="rx_pack"):
        assert F.normalised(a) and F.value(a) < 1 << 256, f"{what}: {a}"
        return F.value(a)

    def store(self, a, what="rx_pack_canonical"):
        self._norm2r(a, what)
        v = F.value(a)
        return v - r if v >= r else v

    def both_branches(self):
        return False

    def acc0(self):  # rx_zero, the start of an accumulation
        return F.limbs(0)


class Bd:
    """Inclusive maxima of a row: lower limbs, top limb, value."""
    __slots__ = ("lo", "top", "val")

    def __init__(self, lo, top, val):
        self.lo, self.top, self.val = lo, top, val

    def __repr__(self):
        return f"Bd(lo<2^{self.lo.bit_length()}, top<2^{self.top.bit_length()}, val={self.val / r:.3f}r)"


class Bounds:
    """The same operations on bounds. An operand is whatever the input contract allows."""

    def __init__(self):
        self.max_column = 0
        self.max_limb = 0
        self.max_product = 0  # the largest product value, in units of r^2
        self.sites = {}       # per product site: (largest column bits, largest product in r^2)

    @staticmethod
    def below(k):
        return Bd(MASK, (k * r - 1) >> TOP_SHIFT, k * r - 1)

    def ld(self, w=None):
        return Bd(MASK, (r - 1) >> TOP_SHIFT, r - 1)

    def unpack(self, w=None):
        return self.below(2)  # every LDS value of k_eval_partial is a packed [0, 2r) element

    const = ld

    def _norm2r(self, a, what):
        assert a.lo <= MASK and a.val < 2 * r, f"{what}: operand not normalised below 2r: {a}"

    def _prod(self, pairs, what):
        col, n = 0, 0
        for x, y in pairs:
            assert max(x.lo, x.top, y.lo, y.top) < U32, what
            self.max_limb = max(self.max_limb, x.lo, x.top, y.lo, y.top)
            col += L * max(x.lo, x.top) * max(y.lo, y.top)
            n += x.val * y.val
        col += L * MASK * MASK          # the reduction terms m_i p_j
        col += col >> B                 # the carry of the column below
        assert col < U64, f"{what}: a column accumulator can reach {col} >= 2^64"
        self.max_column = max(self.max_column, col)
        assert n < F.prod_bound, f"{what}: product up to {n / r / r:.2f} r^2 leaves the result above 2r"
        self.max_product = max(self.max_product, n / r / r)
        old = self.sites.get(what, (0, 0))
        self.sites[what] = (max(old[0], col.bit_length()), max(old[1], round(n / r / r, 3)))
        return self.below(2)

    def mul(self, a, b, what="rx_mul"):
        return self._prod([(a, b)], what)

    def mul_add(self, a, b, c, d, what="rx_mul_add"):
        return self._prod([(a, b), (c, d)], what)

    def add(self, a, b, what="rx_add"):
        self._norm2r(a, what), self._norm2r(b, what)
        return self.below(2)

    sub = add

    def sum_u(self, *rows, what="carry-free sum"):
        out = Bd(sum(x.lo for x in rows), sum(x.top for x in rows), sum(x.val for x in rows))
        assert out.lo < U32 and out.top < U32, f"{what}: a limb can leave 32 bits: {out}"
        self.max_limb = max(self.max_limb, out.lo, out.top)
        return out

    def norm(self, a, what="rx_norm"):
        assert a.lo + (a.lo >> B) < U32 and (a.val >> TOP_SHIFT) < U32, what
        return Bd(MASK, a.val >> TOP_SHIFT, a.val)

    def sub_u(self, a, b, cp, what="rx_sub_u"):
        q = borrow_free(cp)
        assert b.lo <= min(q[:-1]) and b.top <= q[-1], f"{what}<{cp}>: a limb can go negative ({b})"
        out = Bd(a.lo + max(q[:-1]), a.top + q[-1], a.val + cp * r)
        assert out.lo < U32 and out.top < U32, what
        self.max_limb = max(self.max_limb, out.lo, out.top)
        return out

    def is_zero(self, a, what="rx_is_zero"):
        self._norm2r(a, what)
        return False

    def pack(self, a, what="rx_pack"):
        assert a.lo <= MASK and a.val < 1 << 256, what
        return None

    def store(self, a, what="rx_pack_canonical"):
        self._norm2r(a, what)
        return None

    def both_branches(self):
        return True

    def acc0(self):  # an accumulator anywhere in its loop: a [0, 2r) element
        return self.below(2)


# ---- the constants the host hands k_quotient (prover.hip quotient_constants), as words
def quotient_constant_words(ch, s_m, vh_inv) -> dict:
    """Plain challenge values -> the stored words: [e] = value R 2^(-5e)."""
    k = ch["range_sep"] ** 2 % r
    return {
        "alpha": word(ch["alpha"]), "rx_alpha2": word(ch["alpha"] ** 2, -1), "range_sep": word(ch["range_sep"]),
        "rx_bg": [word(ch["beta"] * s, -2) for s in s_m], "rx_beta": word(ch["beta"], -2),
        "rx_gamma": word(ch["gamma"], -1), "rx_one_w": word(1, -1), "rx_two_w": word(2, -1),
        "rx_three_w": word(3, -1), "rx_kappa": word(k, -1), "rx_kappa2": word(k ** 2, -1),
        "rx_kappa3": word(k ** 3, -1), "rx_vh": [word(v, -2) for v in vh_inv], "one": word(1),
    }


# ---- the chains, each written once over an algebra A. `w`: the row's words (Bounds ignores them).
def chain_quotient(A, w, K, blk=0, final=True, has_range=True, has_pi=True, cp=3, extra_summands=0,
                   drop_norm=False):
    """k_quotient<final> for one point. w: a b c d z z_next d_next pi l1 element, sel (11), sigma (4).
    cp / extra_summands / drop_norm: the deliberately weakened variants of the model tests."""
    g = (lambda key, j=None: None) if w is None else (lambda key, j=None: w[key] if j is None else w[key][j])
    kc = (lambda key, j=None: None) if K is None else (lambda key, j=None: K[key] if j is None else K[key][j])
    a, b, c, d = (A.ld(g(x)) for x in "abcd")
    z, z_next = A.ld(g("z")), A.ld(g("z_next"))
    sel = [A.ld(g("sel", j)) for j in range(11)]
    t = A.mul(sel[QM], A.mul(a, b))
    lr = A.mul_add(sel[QL], a, sel[QR], b)
    o4 = A.mul_add(sel[QO], c, sel[Q4], d)
    terms = [t, lr, o4, sel[QC]] + [lr] * extra_summands
    t = A.mul(sel[QARITH], A.sum_u(*terms, what="arithmetic terms"), what="q_arith x carry-free terms")
    if has_pi:
        t = A.add(t, A.ld(g("pi")))
    if has_range:
        qr = sel[QRANGE]
        if A.both_branches() or not A.is_zero(qr):
            d_next = A.ld(g("d_next"))
            one, two, three = (A.const(kc(x)) for x in ("rx_one_w", "rx_two_w", "rx_three_w"))
            dl = lambda f: A.mul(A.mul(f, A.sub(f, one)), A.mul(A.sub(f, two), A.sub(f, three)))
            four = lambda x: A.add(A.add(x, x), A.add(x, x))
            rr = dl(A.sub(c, four(d)))
            rr = A.add(rr, A.mul(dl(A.sub(b, four(c))), A.const(kc("rx_kappa"))))
            rr = A.add(rr, A.mul(dl(A.sub(a, four(b))), A.const(kc("rx_kappa2"))))
            rr = A.add(rr, A.mul(dl(A.sub(d_next, four(a))), A.const(kc("rx_kappa3"))))
            t = A.add(t, A.mul(A.mul(rr, qr), A.const(kc("range_sep"))))
    bX = A.mul(A.const(kc("rx_bg", blk)), A.ld(g("element")))
    bX2 = A.add(bX, bX)
    bX4 = A.add(bX2, bX2)
    bX8 = A.add(bX4, bX4)
    bX16 = A.add(bX8, bX8)
    bX7, bX13, bX17 = A.sub(bX8, bX), A.add(A.add(bX8, bX4), bX), A.add(bX16, bX)
    gm = A.const(kc("rx_gamma"))
    second = "rx_mul with an add3_u second factor"
    first = A.sum_u(a, bX, gm)
    ident = A.mul(first if drop_norm else A.norm(first), A.sum_u(b, bX7, gm), what=second)
    ident = A.mul(ident, A.sum_u(c, bX13, gm), what=second)
    ident = A.mul(ident, A.sum_u(d, bX17, gm), what=second)
    ident = A.mul(ident, z)
    be = A.const(kc("rx_beta"))
    sg = [A.ld(g("sigma", j)) for j in range(4)]
    cpy = A.norm(A.sum_u(a, A.mul(be, sg[0]), gm))
    for wv, s in zip((b, c, d), sg[1:]):
        cpy = A.mul(cpy, A.sum_u(wv, A.mul(be, s), gm), what=second)
    cpy = A.mul(cpy, z_next)
    zm1l1 = A.mul(A.sub_u(z, A.const(kc("one")), cp, what="z - 1"), A.ld(g("l1")))
    perm = A.mul_add(A.sub_u(ident, cpy, cp, what="id - cp"), A.const(kc("alpha")), zm1l1,
                     A.const(kc("rx_alpha2")), what="alpha (id - cp) + alpha^2 (z - 1) L1")
    if final:
        return A.store(A.mul(A.sum_u(t, perm, what="t + perm"), A.const(kc("rx_vh", blk)), what="(t + perm) / v_h"))
    return A.store(A.add(t, perm))


def chain_perm_numden(A, w, K):
    """w: wires (4), sigmas (4), element; K: beta_rx gamma k_rx (3) fix."""
    g = (lambda key, j=None: None) if w is None else (lambda key, j=None: w[key] if j is None else w[key][j])
    kc = (lambda key, j=None: None) if K is None else (lambda key, j=None: K[key] if j is None else K[key][j])
    be, gm = A.const(kc("beta_rx")), A.const(kc("gamma"))
    bx = A.mul(be, A.ld(g("element")))
    second = "rx_mul with an add3_u second factor"
    tn = lambda col, bxk: A.sum_u(A.ld(g("wires", col)), gm, bxk)
    td = lambda col: A.sum_u(A.ld(g("wires", col)), gm, A.mul(be, A.ld(g("sigmas", col))))
    nu, de = A.norm(tn(0, bx)), A.norm(td(0))
    for col in (1, 2, 3):
        nu = A.mul(nu, tn(col, A.mul(A.const(kc("k_rx", col - 1)), bx)), what=second)
        de = A.mul(de, td(col), what=second)
    f = A.const(kc("fix"))
    return A.store(A.mul(nu, f)), A.store(A.mul(de, f))


def perm_constant_words(beta, gamma, ks=(7, 13, 17)) -> dict:
    return {"beta_rx": word(beta, -1), "gamma": word(gamma), "k_rx": [word(k, -1) for k in ks],
            "fix": pow(2, 4 * B * L - 3 * 256, r)}


def chain_coset_combine(A, blocks, vals=None, mat=None):
    """One coefficient index: vals the blocks' words (R domain), mat the rows' words (R')."""
    rr = [A.ld(None if vals is None else vals[m]) for m in range(blocks)]
    out = []
    for l in range(blocks):
        row = [A.const(None if mat is None else mat[l][m]) for m in range(blocks)]
        e = A.mul_add(rr[0], row[0], rr[1], row[1])
        for m in range(2, blocks - 1, 2):
            e = A.add(e, A.mul_add(rr[m], row[m], rr[m + 1], row[m + 1]))
        if blocks & 1:
            e = A.add(e, A.mul(rr[blocks - 1], row[blocks - 1]))
        out.append(A.store(e))
    return out


def chain_pi_sparse(A, count, l1=None, v=None):
    acc = A.mul(A.ld(None if l1 is None else l1[0]), A.const(None if v is None else v[0]))
    for k in range(1, count):
        acc = A.add(acc, A.mul(A.ld(None if l1 is None else l1[k]), A.const(None if v is None else v[k])))
    return A.store(acc)


def chain_lincomb(A, terms, s=None, p=None):
    """s: the scalars' R'-domain words; p: the terms' words at this index (None: past its end)."""
    acc = A.acc0()
    for t in range(terms):
        if p is None or p[t] is not None:
            acc = A.add(acc, A.mul(A.const(None if s is None else s[t]), A.ld(None if p is None else p[t])))
    return A.store(acc)


EVAL_THREADS, EVAL_PER = 256, 16


def chain_eval_block(A, coef=None, x_rx=None, block=0, threads=EVAL_THREADS, per=EVAL_PER):
    """One workgroup of k_eval_partial: the block's coefficient words (at most threads * per; None:
    bounds only, a full block), the point's R'-domain word, the block index. `threads` a power of two
    (the device uses 256; the concrete tests may run a smaller workgroup of the same code)."""
    lg = threads.bit_length() - 1
    t = A.const(x_rx)
    xp = []
    for _ in range(lg + 1):
        xp.append(A.pack(t))
        t = A.mul(t, t, what="rx_sqr")
    for _ in range((threads * per).bit_length() - 1 - (lg + 1)):
        t = A.mul(t, t, what="rx_sqr")
    if x_rx is None:  # pow_blocks_rx: every step multiplies two [0, 2r) values
        rb = A.mul(A.acc0(), t)
        A.mul(t, t, what="rx_sqr")
    else:
        rb, sq, bb = A.const(F.one), t, block
        while bb:
            if bb & 1:
                rb = A.mul(rb, sq)
            sq = A.mul(sq, sq, what="rx_sqr")
            bb >>= 1
    xblock = A.pack(rb)
    x256 = A.unpack(xp[lg])
    n = threads * per if coef is None else len(coef)
    sh = []
    for tid in range(threads if coef is not None else 1):
        acc = A.acc0()
        for i in range(per - 1, -1, -1):
            j = tid + i * threads
            acc = A.mul(acc, x256)
            if j < n:
                acc = A.add(acc, A.ld(None if coef is None else coef[j]))
        sh.append(A.pack(acc))
    if coef is None:  # one fold step carries every step's bounds
        A.pack(A.add(A.unpack(None), A.mul(A.unpack(None), A.unpack(None))))
        return A.store(A.mul(A.unpack(None), A.unpack(None)))
    for l in range(lg - 1, -1, -1):
        h = 1 << l
        for tid in range(h):
            sh[tid] = A.pack(A.add(A.unpack(sh[tid]), A.mul(A.unpack(sh[tid + h]), A.unpack(xp[l]))))
    return A.store(A.mul(A.unpack(sh[0]), A.unpack(xblock)))


def propagate_all() -> dict:
    """The bound propagation of every modelled chain from the input contract. Returns, per chain,
    the largest column accumulator, limb and product value (in r^2) seen."""
    out = {}

    def run(name, fn):
        A = Bounds()
        fn(A)
        out[name] = {"max_column_bits": A.max_column.bit_length(), "max_limb_bits": A.max_limb.bit_length(),
                     "max_product_r2": A.max_product}

    run("k_quotient<true>", lambda A: chain_quotient(A, None, None, final=True))
    run("k_quotient<false>", lambda A: chain_quotient(A, None, None, final=False))
    run("k_perm_numden", lambda A: chain_perm_numden(A, None, None))
    run("k_coset_combine<5>", lambda A: chain_coset_combine(A, 5))
    run("k_coset_combine<6>", lambda A: chain_coset_combine(A, 6))
    run("k_pi_sparse", lambda A: chain_pi_sparse(A, 4))
    run("k_lincomb", lambda A: chain_lincomb(A, 24))
    run("k_eval_partial", lambda A: chain_eval_block(A))
    return out


# ========================================================================== operand pools
MAX_LOW = (1 << TOP_SHIFT) - 1                    # the eight low 29-bit limbs all 2^29 - 1
MAX_LOW_TOPS = (r - 1 - MAX_LOW >> TOP_SHIFT) + 1  # top limbs 0 .. MAX_LOW_TOPS - 1 keep it below r


def max_low_value(top: int) -> int:
    assert 0 <= top < MAX_LOW_TOPS
    return MAX_LOW + (top << TOP_SHIFT)


def canonical_pools(max_low_samples: int = 64) -> dict:
    """The pools of canonical operand values (all below r) that the stage tests draw from. The
    values whose eight low limbs are all 2^29 - 1 exist for MAX_LOW_TOPS (about 2^23) top limbs:
    the pool holds the smallest two, the largest two and max_low_samples evenly spaced ones."""
    half = (r - 1) // 2
    small = [0, 1, 2, 3, r - 1, r - 2, half, half + 1]
    tops = sorted({0, 1, MAX_LOW_TOPS - 2, MAX_LOW_TOPS - 1,
                   *(k * (MAX_LOW_TOPS - 1) // (max_low_samples - 1) for k in range(max_low_samples))})
    max_low = [max_low_value(t) for t in tops]
    assert max_low[-1] < r <= max_low[-1] + (1 << TOP_SHIFT)
    edges = [F.value(row) for row in R.value_edges("fr") + R.limb_edges("fr")]
    edges = sorted({v for v in edges if v < r})
    alt = [F.value(tuple(MASK if i % 2 == ph else 0 for i in range(L - 1)) + (0,)) for ph in (0, 1)]
    single = [MASK << (B * i) for i in range(L - 1)]
    rng = random.Random(0x51A6E)
    rand = [rng.randrange(r) for _ in range(2000)]
    assert all(v < r for v in alt + single + max_low)
    return {"small": small, "max_low": max_low, "edges": edges, "alt": alt, "single": single, "random": rand}


def pool_values() -> list:
    """Every pool, concatenated (the draws are uniform over this list, so an edge value is as
    likely as all random values together are not: see draw())."""
    p = canonical_pools()
    return p["small"] + p["edges"] + p["alt"] + p["single"] + p["max_low"] + p["random"]


def draw(rng: random.Random, count: int, edge_share: float = 0.5) -> list:
    """count operands, each independently an edge value (any non-random pool) with probability
    edge_share, else one of the 2 000 random values."""
    p = canonical_pools()
    edge = p["small"] + p["edges"] + p["alt"] + p["single"] + p["max_low"]
    return [rng.choice(edge) if rng.random() < edge_share else rng.choice(p["random"]) for _ in range(count)]


def extremes() -> list:
    """The values every operand of an all-the-same row takes."""
    p = canonical_pools()
    return [0, 1, r - 1, r - 2, p["max_low"][-1], p["max_low"][0], p["alt"][0], p["alt"][1]]


# ============================================================= words <-> the ABI's arrays
def to_np(words):
    """Stored words (Python integers below 2^256) -> uint64[n, 4], the ABI layout."""
    import numpy as np
    buf = b"".join(w.to_bytes(32, "little") for w in words)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).copy()


def from_np(arr) -> list:
    buf = arr.tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


def words_np(vals, e: int = 0):
    """Plain values -> the stored words at exponent e, as an ABI array."""
    k = MONT * pow(32, -e, r) % r
    return to_np([v * k % r for v in vals])
