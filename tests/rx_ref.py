"""Python-integer reference of the redundant-limb field (csrc/ffr.hpp) and the operand sets of
tests/test_rx_gpu.py and tests/test_g1r_gpu.py.

The reference is the arithmetic's definition, not the limb algorithm: a limb row's value is
sum(v_i 2^(B i)) with the top limb taken whole, and a Montgomery product of N = a b (+ c d) has
ONE exact answer, (N + ((-N p^-1) mod R') p) / R' with R' = 2^(B L) (the digits m_k of the
column algorithm are the base-2^B digits of that m, whatever the order and grouping of the
partial products), so device results are compared limb for limb with that value's unique
normalised limbs. Sums and differences are exact integers."""
from __future__ import annotations

import functools
import random

import pyref as P


class RxField:
    def __init__(self, name: str, p: int, L: int, B: int, N: int, kmax: int):
        self.name, self.p, self.L, self.B, self.N, self.kmax = name, p, L, B, N, kmax
        self.mask = (1 << B) - 1
        self.Rp = 1 << (B * L)
        self.ninv = pow(-p, -1, self.Rp)  # -p^-1 mod R'
        self.one = self.Rp % p
        self.prod_bound = (self.Rp // p) * p * p  # N below it: N / R' + p < 2p (Fp: 630 p^2)
        self.p_limbs = self.limbs(p)

    def value(self, row) -> int:
        return sum(int(v) << (self.B * i) for i, v in enumerate(row))

    def limbs(self, v: int) -> tuple:
        """The normalised limbs of v >= 0: limbs below the top are < 2^B, the top takes the rest."""
        assert v >= 0
        top = v >> (self.B * (self.L - 1))
        assert top < 1 << 32, "value does not fit a limb row"
        return tuple((v >> (self.B * i)) & self.mask for i in range(self.L - 1)) + (top,)

    def normalised(self, row) -> bool:
        return all(int(v) <= self.mask for v in row[:-1])

    def mont(self, n: int) -> int:
        """(n + m p) / R' with m = -n p^-1 mod R': the Montgomery reduction's exact result."""
        t = n + ((n * self.ninv) % self.Rp) * self.p
        assert t & (self.Rp - 1) == 0
        return t >> (self.B * self.L)

    def top_of(self, v: int) -> int:
        return v >> (self.B * (self.L - 1))


FP = RxField("fp", P.P_MOD, 13, 30, 12, 12)
FR = RxField("fr", P.R_MOD, 9, 29, 8, 21)
FIELDS = {"fp": FP, "fr": FR}
TOP_BITS = 26  # RxPlan: operand top limbs stay below 2^26


# ------------------------------------------------------------------------------ operand rows
def max_limb_rows(F: RxField) -> list:
    """All lower limbs 2^B - 1 under the top limbs of the bounds the code works with."""
    p = F.p
    tops = [0, 1, F.top_of(2 * p - 1), F.top_of(8 * p - 1), F.top_of(12 * p - 1), (1 << TOP_BITS) - 1]
    return [(F.mask,) * (F.L - 1) + (t,) for t in tops]


@functools.lru_cache(maxsize=None)
def value_edges(name: str) -> tuple:
    F = FIELDS[name]
    p = F.p
    vals = {0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p}
    for k in range(1, F.kmax + 1):
        vals |= {k * p - 1, k * p, k * p + 1}
    for j in range(1, F.L):
        vals |= {(1 << (F.B * j)) - 1, 1 << (F.B * j)}
    return tuple(F.limbs(v) for v in sorted(vals))


@functools.lru_cache(maxsize=None)
def limb_edges(name: str) -> tuple:
    F = FIELDS[name]
    L, m = F.L, F.mask
    top = (1 << TOP_BITS) - 1
    rows = max_limb_rows(F)
    for phase in (0, 1):  # alternating 0 and 2^B - 1
        rows.append(tuple(m if i % 2 == phase else 0 for i in range(L - 1)) + (top if (L - 1) % 2 == phase else 0,))
    for i in range(L - 1):  # a single limb at 2^B - 1
        rows.append(tuple(m if k == i else 0 for k in range(L)))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def edge_rows(name: str) -> tuple:
    """Value edges and limb edges, every row normalised with a top limb below 2^26."""
    rows = tuple(dict.fromkeys(value_edges(name) + limb_edges(name)))
    F = FIELDS[name]
    assert all(F.normalised(r) for r in rows)
    return rows


@functools.lru_cache(maxsize=None)
def core_rows(name: str) -> tuple:
    """The rows crossed in triples and quadruples: the max-limb rows, the alternating rows and
    the value bounds, so that every operand position of a group sees a max-limb row."""
    F = FIELDS[name]
    p = F.p
    ml = max_limb_rows(F)
    alt = limb_edges(name)[len(ml):len(ml) + 2]
    vals = [0, 1, p, 2 * p - 1, 12 * p - 1]
    return tuple(dict.fromkeys([ml[5], ml[4], ml[3], ml[2], ml[0], *alt, *(F.limbs(v) for v in vals)]))


@functools.lru_cache(maxsize=None)
def random_rows(name: str, per_range: int = 2000) -> tuple:
    F = FIELDS[name]
    rng = random.Random(0x5EED + F.L)
    return tuple(F.limbs(rng.randrange(k * F.p)) for k in (2, 8, 12) for _ in range(per_range))


def shuffled(rows, seed: int) -> list:
    out = list(rows)
    random.Random(seed).shuffle(out)
    return out


def cross(rows, arity: int) -> list:
    """arity lists: the full cross product of rows, column by column."""
    n = len(rows)
    cols = []
    for k in range(arity):
        rep = n ** (arity - 1 - k)
        cols.append([rows[(i // rep) % n] for i in range(n ** arity)])
    return cols


@functools.lru_cache(maxsize=None)
def fr_unnormalised_rows() -> tuple:
    """The unnormalised first factors the NTT gives rx_mul and twmul2 (csrc/ntt.hip), with their
    documented bounds: (rows with limbs up to 2^31.6 and values below 21r, as sub_u2<11> gives
    them; rows with limbs below 2^29 + 2^30 and values below 5r, as rx_sub_u<FrCfg, 3> does)."""
    F = FR
    r, L, B = F.p, F.L, F.B
    rng = random.Random(31)
    big, small = [], []
    lim = int(2 ** 31.6)  # the comment's limb bound
    # every limb at the bound; the top limb as large as the value bound 21r allows
    low = sum((lim - 1) << (B * i) for i in range(L - 1))
    big.append((lim - 1,) * (L - 1) + ((21 * r - 1 - low) >> (B * (L - 1)),))
    big.append((lim - 1,) * (L - 1) + (0,))
    # a + 11r - b limb by limb with 11r's lower limbs raised by 2^30 (sub_u2<11>): a normalised
    # below 5r, b the limb-wise sum of two normalised values below 5r
    q11 = list(F.limbs(11 * r))
    q11[0] += 2 << B
    for i in range(1, L - 1):
        q11[i] += (2 << B) - 2
    q11[L - 1] -= 2
    edge5 = [F.limbs(v) for v in (0, 1, r - 1, r, 2 * r - 1, 5 * r - 1)] + [(F.mask,) * (L - 1) + (0,)]
    for _ in range(300):
        a = rng.choice(edge5) if rng.random() < 0.5 else F.limbs(rng.randrange(5 * r))
        b1 = rng.choice(edge5) if rng.random() < 0.5 else F.limbs(rng.randrange(5 * r))
        b2 = rng.choice(edge5) if rng.random() < 0.5 else F.limbs(rng.randrange(5 * r))
        big.append(tuple(a[i] + q11[i] - b1[i] - b2[i] for i in range(L)))
    # a + 3r - b with 3r borrow-free (rx_sub_u<FrCfg, 3>): a, b normalised below 2r
    q3 = list(F.limbs(3 * r))
    q3[0] += 1 << B
    for i in range(1, L - 1):
        q3[i] += (1 << B) - 1
    q3[L - 1] -= 1
    edge2 = [F.limbs(v) for v in (0, 1, r - 1, r, r + 1, 2 * r - 1)] + [(F.mask,) * (L - 1) + (0,)]
    for a in edge2:
        for b in edge2:
            small.append(tuple(a[i] + q3[i] - b[i] for i in range(L)))
    lim3 = (1 << B) + (2 << B) - 1
    low = sum(lim3 << (B * i) for i in range(L - 1))
    small.append((lim3,) * (L - 1) + ((5 * r - 1 - low) >> (B * (L - 1)),))
    return tuple(big), tuple(small)


def fr_max_limb_seconds() -> tuple:
    """Normalised second factors below 2r with every lower limb at 2^29 - 1."""
    F = FR
    rows = tuple((F.mask,) * (F.L - 1) + (t,) for t in (0, 1, F.top_of(2 * F.p - 1) - 1))
    assert all(F.value(r) < 2 * F.p for r in rows)
    return rows


# ------------------------------------------------------------------- the unsplit column bound
def unsplit_mul_add_max_column(F: RxField, a, b, c, d) -> int:
    """The largest value a single accumulator per column would hold in rx_mul_add(a, b, c, d)
    (carry + both product sets + the reduction terms of the column), in Python integers."""
    L, B, pl = F.L, F.B, F.p_limbs
    ninv0 = F.ninv & F.mask
    m, acc, worst = [], 0, 0
    for k in range(2 * L - 1):
        for i in range(max(0, k - L + 1), min(k, L - 1) + 1):
            acc += a[i] * b[k - i] + c[i] * d[k - i]
            if i < k or k >= L:
                acc += m[i] * pl[k - i]
        if k < L:
            m.append((acc * ninv0) & F.mask)
            acc += m[k] * pl[0]
        worst = max(worst, acc)
        acc >>= B
    return worst


# ------------------------------------------------------------------------------- G1 in XYZZ
def xyzz_row(pt, z: int, lifts) -> tuple:
    """The R'-domain XYZZ limbs of the affine point pt under z (ZZ = z^2, ZZZ = z^3), each
    coordinate raised by lifts[i] * p."""
    F, p = FP, FP.p
    x, y = pt
    zz, zzz = z * z % p, z * z * z % p
    vals = (x * zz, y * zzz, zz, zzz)
    return tuple(F.limbs(v * F.Rp % p + k * p) for v, k in zip(vals, lifts))


def xyzz_decode(row):
    """(affine point or None, ZZ^3 == ZZZ^2) of a device XYZZ row; infinity is ZZ in {0, p}."""
    F, p = FP, FP.p
    X, Y, ZZ, ZZZ = (F.value(c) for c in row)
    if ZZ in (0, p):
        return None, True
    rinv = pow(F.Rp, -1, p)
    zz, zzz = ZZ * rinv % p, ZZZ * rinv % p
    pt = (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)
    return pt, pow(zz, 3, p) == zzz * zzz % p
