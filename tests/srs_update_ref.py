"""Python-integer reference of the SRS update (include/plk.h "Updating an SRS"): the scalar split
of csrc/g1_mul.hip, a model of its addition chain on oracle/pyref.py's group law, and the scalar
lists the CPU and GPU tests share.

z = x0^2 with x0 = 0xd201000000010000 (the BLS parameter's absolute value); r = z^2 - z + 1;
psi(x, y) = (beta x, y) = [-z](x, y) on G1.
"""
import numpy as np

import pyref as P

p, r = P.P_MOD, P.R_MOD
X0 = 0xD201000000010000
Z = X0 * X0
assert Z == 0xAC45A4010001A4020000000100000000 and r == Z * Z - Z + 1 and (r - 1) // Z == Z - 1
# beta: the cube root of unity with (beta x, y) = [-z](x, y); fixed by the check in chain_mul's test
BETA = 0x5F19672FDF76CE51BA69C6076A0F77EADDB3A93BE6F89688DE17D813620A00022E01FFFFFFFEFFFE
assert pow(BETA, 3, p) == 1 and BETA != 1


def split(k: int):
    """(a, b) with a = z - (k mod z), b = k // z + 1: both in [1, z], a - b z = -k."""
    return Z - k % Z, k // Z + 1


def psi(pt):
    return None if pt is None else (BETA * pt[0] % p, pt[1])


def chain_mul(pt, k: int):
    """[k] pt the way k_g1_mul walks: 128 doublings, the digit (bit of a, bit of b) picking
    -P, -psi P or -(P + psi P) = (beta^2 x, y)."""
    if pt is None:
        return None
    a, b = split(k)
    x, y = pt
    table = {1: (x, p - y), 2: (BETA * x % p, p - y), 3: (BETA * BETA * x % p, y)}
    acc = None
    for i in range(127, -1, -1):
        acc = P.g1_add(acc, acc)
        d = ((a >> i) & 1) | (((b >> i) & 1) << 1)
        if d:
            acc = P.g1_add(acc, table[d])
    return acc


def edge_scalars():
    """Where a quotient digit of the division by z could be off by one, and the ends of the range."""
    out = [0, 1, 2, Z - 1, Z, Z + 1, 2 * Z - 1, 2 * Z]
    for m in ((1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 64, 1 << 96, 1 << 127, Z - 1):
        out += [v for v in (m * Z - 1, m * Z, m * Z + 1) if v < r]
    out += [(1 << 128) - 1, 1 << 128, 1 << 192, 1 << 254, r - 2, r - 1]
    return out


def random_scalars(count: int, seed: int):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [int.from_bytes(rng.bytes(40), "little") % r for _ in range(count)]


def split_rows(scalars) -> np.ndarray:
    """uint64[n, 4]: a_lo, a_hi, b_lo, b_hi, as plk_debug_glv_split writes them."""
    m = (1 << 64) - 1
    rows = []
    for k in scalars:
        a, b = split(k)
        rows.append([a & m, a >> 64, b & m, b >> 64])
    return np.array(rows, dtype=np.uint64)
