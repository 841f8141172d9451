"""Pure-Python reference of the ingest stage (include/plk.h "Compact proofs and the ingest
stage"): zkcrypto's 48-byte compressed G1, its strict decoding with the status codes of the
batched calls, the compact proof layout, and G1 membership.

Built on oracle/pyref.py's jac_* functions. Membership is decided as [r]P == O with an unreduced
double-and-add of its own (pyref.g1_mul reduces its scalar mod r, so g1_mul(Q, r) is the
identity for every curve point), independent of the endomorphism test the library runs.
"""
import numpy as np

import pyref as P

p = P.P_MOD
r = P.R_MOD
OK, ENCODING, RANGE, OFF_CURVE, SUBGROUP = range(5)
G1_BYTES, FR_BYTES, COMPACT_BYTES = 48, 32, 11 * 48 + 16 * 32

# the cofactor of G1: #E(Fp) = H * r
H = 0x396C8C005555E1568C00AAAB0000AAAB
H_PRIMES = (3, 11, 10177, 859267, 52437899)
assert H == 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2


def mul(pt, k: int):
    """[k] pt for any non-negative integer k (never reduced) -> affine / None."""
    acc = (1, 1, 0)
    base = P.jac_from_affine(pt)
    for bit in bin(k)[2:] if k else "":
        acc = P.jac_double(acc)
        if bit == "1":
            acc = P.jac_add(acc, base)
    return P.jac_to_affine(acc)


def in_subgroup(pt) -> bool:
    """pt (on the curve, or None) has order dividing r."""
    return mul(pt, r) is None


def sqrt(a: int):
    """A square root of a mod p (p = 3 mod 4), or None."""
    y = pow(a, (p + 1) // 4, p)
    return y if y * y % p == a % p else None


def has_point(x: int) -> bool:
    return sqrt((x ** 3 + 4) % p) is not None


def compress(pt) -> bytes:
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    x, y = pt
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80
    if y > (p - 1) // 2:
        b[0] |= 0x20
    return bytes(b)


def raw48(x: int, flags: int) -> bytes:
    """48 bytes with any 381-bit x and any flag bits (0x80 compressed, 0x40 infinity, 0x20 sort)."""
    b = bytearray(x.to_bytes(48, "big"))
    assert b[0] < 0x20
    b[0] |= flags
    return bytes(b)


def decompress(b: bytes, subgroup: bool = True):
    """(status, point): the strict decoding. point is None unless status == OK and the point is
    finite; identity tells the two apart."""
    assert len(b) == 48
    if not b[0] & 0x80:
        return ENCODING, None, False
    if b[0] & 0x40:
        if b != bytes([0xC0]) + bytes(47):
            return ENCODING, None, False
        return OK, None, True
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")
    if x >= p:
        return RANGE, None, False
    y = sqrt((x ** 3 + 4) % p)
    if y is None:
        return OFF_CURVE, None, False
    if (y > (p - 1) // 2) != bool(b[0] & 0x20):
        y = p - y
    if subgroup and not in_subgroup((x, y)):
        return SUBGROUP, None, False
    return OK, (x, y), False


def decompress_words(b: bytes, subgroup: bool = True):
    """(status, uint64[13]) as the library returns them: zero words for a rejected point."""
    st, pt, ident = decompress(b, subgroup)
    if st != OK:
        return st, np.zeros(13, dtype=np.uint64)
    return st, P.g1_vec_to_np([None if ident else pt])[0]


def random_curve_point(rng):
    """A uniformly drawn curve point (almost never of order r)."""
    while True:
        x = int.from_bytes(rng.bytes(48), "big") % p
        y = sqrt((x ** 3 + 4) % p)
        if y is not None:
            return (x, y if rng.integers(2) else p - y)


def low_order_point(q: int, rng):
    """A point of order exactly q (q a prime of the cofactor) from a random curve point Q,
    redrawn when it comes out as the identity: T = [r h / q^e] Q with q^e the full power of q in
    h, multiplied by q until [q] T = O. ([r h / q] Q alone is always the identity for the four
    squared primes: E(Fp) is Z_m x Z_3mr with m = 11 * 10177 * 859267 * 52437899, its q-part is
    Z_q x Z_q and the group's exponent r h / m already kills it.)"""
    assert H % q == 0
    qe = q * q if H % (q * q) == 0 else q
    while True:
        t = mul(random_curve_point(rng), r * H // qe)
        if t is None:
            continue
        while mul(t, q) is not None:
            t = mul(t, q)
        return t


def member(k: int):
    """[k] G, a point of G1."""
    return P.g1_mul(P.G1_GEN, k)


def non_member(q: int, rng, k: int = 5):
    """G' + T with G' = [k] G in G1 and T of order q: on the curve, outside G1."""
    return P.g1_add(member(k), low_order_point(q, rng))


def proof_to_compact(comm_points, evals) -> bytes:
    """11 affine points (None = identity) and 16 canonical scalars -> the compact bytes."""
    assert len(comm_points) == 11 and len(evals) == 16
    return b"".join(compress(c) for c in comm_points) + b"".join(
        int(e).to_bytes(32, "little") for e in evals)


def scalar_status(b: bytes) -> int:
    return RANGE if int.from_bytes(b, "little") >= r else OK


def proof_status(data: bytes, subgroup: bool = True) -> int:
    """The first failing code over the 27 fields of one compact proof."""
    assert len(data) == COMPACT_BYTES
    for i in range(11):
        st = decompress(data[48 * i: 48 * i + 48], subgroup)[0]
        if st != OK:
            return st
    for i in range(16):
        st = scalar_status(data[528 + 32 * i: 528 + 32 * i + 32])
        if st != OK:
            return st
    return OK


# ---- the rules every entry point that validates plk_g1 input shares (plk_msm_points' contract) ---
ABI_REFUSED = ("infinity word 2", "x = p", "y = 2p - y0", "off the curve")
ABI_IDENTITY = "identity with garbage"
ABI_LANES = (0, 63, 64)  # first lane, last lane of a wave, first lane of the second wave


def abi_spoil(row, what: str) -> np.ndarray:
    """A copy of the finite ABI row uint64[13] (Montgomery limbs) turned into one of the malformed
    points of ABI_REFUSED (every one refused with PLK_E_ARG) or into ABI_IDENTITY (infinity word 1
    over arbitrary coordinate words: accepted as the identity)."""
    row = np.array(row, dtype=np.uint64)
    assert row.shape == (13,) and row[12] == 0
    y0 = P.limbs_to_int(row[6:12])
    if what == "infinity word 2":
        row[12] = 2
    elif what == "x = p":  # the limbs of p itself: the smallest value that is not canonical
        row[:6] = np.array(P.int_to_limbs(p, 6), dtype=np.uint64)
    elif what == "y = 2p - y0":  # -y0 mod p, so on the curve as a residue, but >= p as limbs
        assert p <= 2 * p - y0 < 1 << 384
        row[6:12] = np.array(P.int_to_limbs(2 * p - y0, 6), dtype=np.uint64)
    elif what == "off the curve":  # canonical; y0 + 1 = -y0 has no solution beside y0 = (p - 1) / 2
        assert 2 * y0 + 1 != p
        row[6:12] = np.array(P.int_to_limbs((y0 + 1) % p, 6), dtype=np.uint64)
    elif what == ABI_IDENTITY:  # words >= p, a canonical residue, zero: none of them is looked at
        row[:12] = np.array([0xFFFFFFFFFFFFFFFF] * 6 + [0xDEADBEEF, 1, 2, 3, 0, 5], dtype=np.uint64)
        row[12] = 1
    else:
        raise ValueError(what)
    return row
