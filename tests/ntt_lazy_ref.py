"""Python-integer model of the lazy butterfly helpers of the NTT pass kernel (csrc/ntt.hip:
add_u, sub_u, rx_sub_u<5/6>, sub_u2<11>, reduce_q over kZTab, r4_math<H1>, the in-register first
stage and the twiddle-free last stage of odd radices, the three store forms) on exact limb rows
of rx_ref.FR, and the operand sets of tests/test_ntt_lazy.py.

Every step asserts what the device code relies on: every intermediate limb fits 32 bits (nothing
wraps), reduce_q's table index is below kQMax and its result is exactly value(a) - q r >= 0 with
normalised limbs, every product keeps its columns below 2^64 and its operands inside rx_mul's Fr
contract. The `check_*` functions are the preconditions written at each consumer in ntt.hip; a
helper's output is checked against its consumer's precondition by the caller (the induction over
the stages of a pass: inputs of r4_math and of the odd stages normalised below 5r, the store's
input normalised below 5r, rx_pack_canonical's below 2r).

A product is the one exact Montgomery value (rx_ref.RxField.mont), as in tests/test_rx_gpu.py,
which pins rx_mul / rx_mul2 against it on the same operand classes.

Model(strict=False) computes what 32-bit and 64-bit registers would hold instead of asserting
(limbs mod 2^32, columns mod 2^64) and records every reduce_q index: it is how the effect of a
changed constant is studied (Model.cp overrides the multiples of r of the lazy subtractions)."""
from __future__ import annotations

import functools
import random

import rx_ref as R

F = R.FR
r = F.p
L, B, MASK = F.L, F.B, F.mask
K_QMAX = 32                      # ntt.hip kQMax: q of a value below 2^260
Q_SHIFT = 255 - B * (L - 1)      # q = top limb >> 23
LIMB_U = int(2 ** 31.6)          # the limb bound of an unnormalised multiplicand / reduce_q input
ZERO = (0,) * L
U32, U64 = 1 << 32, 1 << 64


@functools.lru_cache(maxsize=None)
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


@functools.lru_cache(maxsize=None)
def raised2(c: int) -> tuple:
    """ntt.hip FrRaised2<c>: c r with every limb below the top raised by 2^(B+1) - 2 (2^(B+1) for
    limb 0)."""
    m = list(F.limbs(c * r))
    m[0] += 2 << B
    for i in range(1, L - 1):
        m[i] += (2 << B) - 2
    m[L - 1] -= 2
    assert F.value(m) == c * r
    return tuple(m)


def make_ztab() -> tuple:
    """kZTab: row q holds the normalised limbs of 2^261 - q r."""
    return tuple(F.limbs((1 << (B * L)) - q * r) for q in range(K_QMAX))


# ------------------------------------------------------------------------- the preconditions
def check_normalised_below(row, k: int, what: str):
    assert F.normalised(row) and 0 <= F.value(row) < k * r, f"{what}: not normalised below {k}r: {row}"


def check_twiddle(row):
    """An R'-domain canonical table entry: normalised, below r."""
    check_normalised_below(row, 1, "twiddle")


def check_reduce_q_input(row):
    """reduce_q: limbs below 2^31.6, value below 2^260."""
    assert all(0 <= v < LIMB_U for v in row) and F.value(row) < 1 << 260, f"reduce_q input {row}"


def check_sum_operand(row):
    """The subtrahend of sub_u2: a limb-wise sum of two normalised values below 5r."""
    assert all(0 <= v <= 2 * MASK for v in row[:-1]) and F.value(row) < 10 * r, f"sum operand {row}"
    assert row[-1] <= 2 * F.top_of(5 * r - 1)


def check_mul_operands(a, b):
    """rx_mul's Fr contract (ffr.hpp rx_sub_u, ntt.hip sub_u2): the first factor's limbs below
    2^31.6, the second normalised below 2r, the product below (R' / r) r^2 so that the result is
    below 2r."""
    assert all(0 <= v < LIMB_U for v in a), f"multiplicand limbs {a}"
    check_normalised_below(b, 2, "second factor")
    assert F.value(a) * F.value(b) < F.prod_bound, "product outside rx_mul's value bound"


class Model:
    """The helpers on limb rows. strict: assert every bound; otherwise wrap like the registers."""

    def __init__(self, strict: bool = True, ztab=None, cp=None):
        self.strict = strict
        self.ztab = ztab if ztab is not None else make_ztab()
        # the multiples of r of the lazy subtractions, by site
        self.cp = {"r4_x02": 6, "r4_x13": 6, "r4_y01": 11, "r4_y23": 5, "r2first": 3, "odd_last": 6}
        self.cp.update(cp or {})
        self.q_seen = []        # reduce_q indices (every call)
        self.max_column = 0
        self.max_limb = 0
        self._products = {}     # (a, b) -> checked product (the cross repeats most of them)

    # ---- limb arithmetic
    def _u32(self, row, what: str) -> tuple:
        """A row of 32-bit registers: strict asserts that nothing wraps."""
        if self.strict:
            lo, hi = min(row), max(row)
            assert 0 <= lo and hi < U32, f"{what}: a limb of {row} leaves 32 bits"
            if hi > self.max_limb:
                self.max_limb = hi
            return tuple(row)
        return tuple(v % U32 for v in row)

    def add_u(self, a, b) -> tuple:
        return self._u32([x + y for x, y in zip(a, b)], "add_u")

    def _sub(self, a, b, q, what) -> tuple:
        t = self._u32([x + m for x, m in zip(a, q)], what)
        return self._u32([x - y for x, y in zip(t, b)], what)

    def rx_sub_u(self, a, b, cp: int) -> tuple:
        return self._sub(a, b, borrow_free(cp), f"rx_sub_u<{cp}>")

    def sub_u(self, a, b) -> tuple:
        return self.rx_sub_u(a, b, self.cp["r2first"])

    def sub_u2(self, a, b, cp: int = 11) -> tuple:
        return self._sub(a, b, raised2(cp), f"sub_u2<{cp}>")

    def reduce_q(self, a) -> tuple:
        q = a[L - 1] >> Q_SHIFT
        self.q_seen.append(q)
        if self.strict:
            check_reduce_q_input(a)
            assert q < K_QMAX, f"reduce_q index {q}"
        elif q >= K_QMAX:
            return None  # the device would read past the table: the caller stops here
        z = self.ztab[q]
        out, c = [], 0
        for i in range(L - 1):
            t = a[i] + z[i] + c
            if not self.strict:
                t %= U32
            elif t >= U32:
                raise AssertionError(f"reduce_q: limb {i} of {a} leaves 32 bits")
            out.append(t & MASK)
            c = t >> B
        t = self._u32([a[L - 1] + z[L - 1] + c], "reduce_q top")[0]
        out = tuple(out) + self._u32([t - (1 << B)], "reduce_q top")
        if self.strict:
            assert F.value(out) == F.value(a) - q * r and F.value(out) >= 0, (a, out)
            assert F.normalised(out)
        return out

    def rx_mul(self, a, b) -> tuple:
        if self.strict:
            hit = self._products.get((a, b))
            if hit is not None:
                return hit
            check_mul_operands(a, b)
            col = R.unsplit_mul_add_max_column(F, a, b, ZERO, ZERO)
            assert col < U64, f"column {col} of {a} x {b}"
            self.max_column = max(self.max_column, col)
            t = F.mont(F.value(a) * F.value(b))
            assert t < 2 * r
            self._products[(a, b)] = F.limbs(t)
            return self._products[(a, b)]
        return mul_columns(a, b)

    twmul = rx_mul

    # ---- the butterflies
    def r4_math(self, h1: bool, x, tw) -> tuple:
        """x: rows x0..x3; tw: (w,) for h1, else (w(r s1), w((r + h) s1), w(r s2))."""
        x0, x1, x2, x3 = x
        y0, y1 = self.add_u(x0, x2), self.add_u(x1, x3)
        d02 = self.rx_sub_u(x0, x2, self.cp["r4_x02"])
        d13 = self.rx_sub_u(x1, x3, self.cp["r4_x13"])
        if h1:
            y2 = self.reduce_q(d02)
            y3 = self.twmul(d13, tw[0])
            if y2 is None:
                return None
            o = (self.reduce_q(self.add_u(y0, y1)), self.reduce_q(self.sub_u2(y0, y1, self.cp["r4_y01"])),
                 self.reduce_q(self.add_u(y2, y3)), self.reduce_q(self.rx_sub_u(y2, y3, self.cp["r4_y23"])))
        else:
            y2, y3 = self.twmul(d02, tw[0]), self.twmul(d13, tw[1])
            o = (self.reduce_q(self.add_u(y0, y1)), self.twmul(self.sub_u2(y0, y1, self.cp["r4_y01"]), tw[2]),
                 self.reduce_q(self.add_u(y2, y3)), self.twmul(self.rx_sub_u(y2, y3, self.cp["r4_y23"]), tw[2]))
        return None if any(v is None for v in o) else o

    def r2first(self, a, v, w) -> tuple:
        return self.reduce_q(self.add_u(a, v)), self.twmul(self.sub_u(a, v), w)

    def odd_last(self, a, c) -> tuple:
        return self.reduce_q(self.add_u(a, c)), self.reduce_q(self.rx_sub_u(a, c, self.cp["odd_last"]))

    # ---- the stores: the packed canonical word as a row (8 words, then 0)
    def pack_canonical(self, v) -> tuple:
        if self.strict:
            check_normalised_below(v, 2, "rx_pack_canonical input")
        x = F.value(v) % (1 << 256)
        if x >= r:  # fe_reduce_once
            x -= r
        return tuple((x >> (32 * i)) & 0xFFFFFFFF for i in range(8)) + (0,)

    def store0(self, v) -> tuple:
        return self.pack_canonical(self.reduce_q(v))

    def store_scaled(self, v, s_words) -> tuple:
        return self.pack_canonical(self.rx_mul(v, unpack_words(s_words)))


def mul_columns(a, b) -> tuple:
    """ffr.hpp rx_mul's column algorithm with a 64-bit accumulator that wraps (Model.strict =
    False; inside the contract it equals the exact Montgomery value)."""
    pl, ninv0 = F.p_limbs, F.ninv & MASK
    m, out, acc = [], [], 0
    for k in range(2 * L - 1):
        for i in range(max(0, k - L + 1), min(k, L - 1) + 1):
            acc += a[i] * b[k - i]
            if i < k or k >= L:
                acc += m[i] * pl[k - i]
        acc %= U64
        if k < L:
            m.append(((acc % U32) * ninv0) & MASK)
            acc = (acc + m[k] * pl[0]) % U64
        else:
            out.append(acc & MASK)
        acc >>= B
    out.append(acc % U32)
    return tuple(out)


def words_of(v: int) -> tuple:
    """A packed value below 2^256 as a hook row: 8 words, then 0."""
    assert 0 <= v < 1 << 256
    return tuple((v >> (32 * i)) & 0xFFFFFFFF for i in range(8)) + (0,)


def unpack_words(row) -> tuple:
    return F.limbs(sum(int(w) << (32 * i) for i, w in enumerate(row[:8])))


def residue(row) -> int:
    return F.value(row) % r


RP_INV = pow(F.Rp, -1, r)


# ------------------------------------------------------------------------------ operand sets
def max_limb_row(top: int) -> tuple:
    return (MASK,) * (L - 1) + (top,)


def alternating_rows(top: int) -> list:
    """Limbs alternating 0 and 2^B - 1, either phase; the top limb position takes `top` or 0."""
    return [tuple(MASK if i % 2 == ph else 0 for i in range(L - 1)) + (top if (L - 1) % 2 == ph else 0,)
            for ph in (0, 1)]


@functools.lru_cache(maxsize=None)
def data_rows(k: int) -> tuple:
    """The data rows of a butterfly whose inputs are normalised below k r (k = 5: r4_math, the
    odd last stage, the stores; k = 2: the first stage of an odd radix): the values at and next
    to every multiple of r in range, rows with every lower limb at 2^B - 1 under the smallest and
    the largest top limb, and the alternating-limb rows."""
    top = F.top_of(k * r - 1)
    vals = [0, 1, r - 1, r, r + 1, 2 * r - 1, 2 * r, 4 * r - 1, 5 * r - 1]
    rows = [F.limbs(v) for v in vals if v < k * r]
    rows += [max_limb_row(0), max_limb_row(top - 1)] + alternating_rows(top - 1)
    rows = tuple(dict.fromkeys(rows))
    for row in rows:
        check_normalised_below(row, k, "data row")
    return rows


def carry_rows(k: int) -> tuple:
    """Rows below k r with every lower limb at 2^B - 1 whose double sits just under an odd
    multiple m of 2^255: the limb-wise sum of two of them has a top limb one short of m << 23 and
    a carry pending below it, so reduce_q's q is one low (the two-row butterflies only)."""
    rows = tuple(max_limb_row((m << (Q_SHIFT - 1)) - 1) for m in (1, 3, 5, 7))
    return tuple(row for row in rows if F.value(row) < k * r)


@functools.lru_cache(maxsize=None)
def twiddle_rows() -> tuple:
    """R'-domain canonical twiddles: 0, 1, R' mod r (the twiddle one), r - 1 and the row with every
    lower limb at 2^B - 1 below r."""
    rows = tuple(F.limbs(v) for v in (0, 1, F.one, r - 1)) + (max_limb_row(F.top_of(r - 1) - 1),)
    for row in rows:
        check_twiddle(row)
    return rows


def twiddle_triples() -> list:
    """Triples of distinct twiddles (every twiddle in every position), then the equal ones."""
    t = twiddle_rows()
    n = len(t)
    tri = [(t[i], t[(i + s) % n], t[(i + 2 * s) % n]) for s in (1, 2) for i in range(n)]
    assert all(len(set(x)) == 3 for x in tri)
    return tri + [(w, w, w) for w in t]


def random_data(k: int, count: int, seed: int) -> list:
    rng = random.Random(seed)
    return [F.limbs(rng.randrange(k * r)) for _ in range(count)]


def random_twiddles(count: int, seed: int) -> list:
    rng = random.Random(seed)
    return [F.limbs(rng.randrange(r)) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def r4_cases(kind: str) -> tuple:
    """(x0..x3, twiddle triple) of r4_math. edges: data_rows(5) crossed fourfold, case i under
    twiddle triple i mod 15 (13^4 and 15 are coprime: every row meets every triple in every
    position many times), then the largest value, the largest max-limb row and 0 crossed
    fourfold under every triple; random: 3 000 random rows below 5r under random twiddles."""
    if kind == "edges":
        cols = R.cross(data_rows(5), 4)
        tri = twiddle_triples()
        cases = [(x, tri[i % len(tri)]) for i, x in enumerate(zip(*cols))]
        top = (F.limbs(5 * r - 1), max_limb_row(F.top_of(5 * r - 1) - 1), F.limbs(0))
        cases += [((a, b, c, d), t) for a in top for b in top for c in top for d in top for t in tri]
        return tuple(cases)
    d = [random_data(5, 3000, 40 + j) for j in range(4)]
    w = [random_twiddles(3000, 50 + j) for j in range(3)]
    return tuple(zip(zip(*d), zip(*w)))


@functools.lru_cache(maxsize=None)
def pair_cases(k: int, kind: str) -> tuple:
    """(a, b, twiddle) of the two-row butterflies with inputs below k r: data_rows(k) crossed with
    (and carry_rows(k)) crossed with itself and with every twiddle, or 3 000 random cases."""
    if kind == "edges":
        rows = data_rows(k) + carry_rows(k)
        return tuple((a, b, w) for a in rows for b in rows for w in twiddle_rows())
    return tuple(zip(random_data(k, 3000, 60 + k), random_data(k, 3000, 61 + k), random_twiddles(3000, 62 + k)))


@functools.lru_cache(maxsize=None)
def reduce_q_rows(kind: str) -> tuple:
    """reduce_q on its own. edges: every q < 32 from a top limb of q << 23 over zero lower limbs
    and over lower limbs all at 2^31 - 1, and the values q r, q r +- 1, (q + 1) 2^255 - 1 and
    q 2^255 that stay in [0, 2^260) (value >= q' r holds for the q' any row gives: r < 2^255).
    random: 3 000 rows of random limbs below 2^31.6 and 1 000 normalised values below 2^260."""
    rows = []
    if kind == "edges":
        for q in range(K_QMAX):
            rows.append((0,) * (L - 1) + (q << Q_SHIFT,))
            rows.append(((1 << 31) - 1,) * (L - 1) + (q << Q_SHIFT,))
            for v in (q * r - 1, q * r, q * r + 1, ((q + 1) << 255) - 1, q << 255):
                if 0 <= v < 1 << 260:
                    rows.append(F.limbs(v))
    else:
        rng = random.Random(77)
        for _ in range(3000):
            rows.append(tuple(rng.randrange(LIMB_U) for _ in range(L - 1)) + (rng.randrange(1 << 28),))
        for _ in range(1000):
            rows.append(F.limbs(rng.randrange(1 << 260)))
    rows = tuple(dict.fromkeys(rows))
    for row in rows:
        check_reduce_q_input(row)
    return rows


@functools.lru_cache(maxsize=None)
def sub_u2_cases(kind: str) -> tuple:
    """(a, b) of sub_u2<11>: limb-wise sums of two rows of data_rows(5) (the y0, y1 of r4_math)."""
    if kind == "edges":
        rows = data_rows(5)
        sums = tuple(dict.fromkeys(tuple(x + y for x, y in zip(p, q)) for p in rows for q in rows))
        keep = sums[:: max(1, len(sums) // 40)] + (sums[-1],)
        big = tuple(tuple(x + y for x, y in zip(p, p)) for p in (max_limb_row(F.top_of(5 * r - 1) - 1), F.limbs(5 * r - 1)))
        keep = tuple(dict.fromkeys(keep + big + (ZERO,)))
        cases = tuple((a, b) for a in keep for b in keep)
    else:
        d = [random_data(5, 3000, 70 + j) for j in range(4)]
        cases = tuple((tuple(x + y for x, y in zip(p, q)), tuple(x + y for x, y in zip(s, t)))
                      for p, q, s, t in zip(*d))
    for a, b in cases:
        check_sum_operand(a)
        check_sum_operand(b)
    return cases


@functools.lru_cache(maxsize=None)
def store_rows(kind: str) -> tuple:
    """The store's inputs (normalised, below 5r). edges: the data rows, every k r and k r +- 1
    below 5r (reduce_q takes them to 0, r and their neighbours: the values fe_reduce_once must
    get right) and the multiples of 2^255 with their neighbours; random: 3 000 rows."""
    if kind == "edges":
        vals = {k * r + d for k in range(6) for d in (-1, 0, 1)}
        vals |= {(q << 255) + d for q in range(1, 5) for d in (-1, 0, 1)}
        rows = data_rows(5) + tuple(F.limbs(v) for v in sorted(vals) if 0 <= v < 5 * r)
    else:
        rows = tuple(random_data(5, 3000, 80))
    rows = tuple(dict.fromkeys(rows))
    for row in rows:
        check_normalised_below(row, 5, "store input")
    return rows


def scale_words() -> tuple:
    """Packed canonical R'-domain scales: the twiddle set's values."""
    return tuple(words_of(F.value(w)) for w in twiddle_rows())
