"""Integer model of the fixed-base MSM's row-table recoding (csrc/msm_digits.hpp naf_walk): the
canonical half h <= (r - 1) / 2 of a scalar as at most ceil(255 / (c + 1)) pairs (bit position,
odd signed digit), sum d 2^pos = h, |d| < 2^c, over a table with one row 2^pos P per bit position.

Two passes. Pass 1 is the greedy width-(c + 1) sliding window (a window starts at a set bit of the
running value, a digit of 2^c and up borrows from above), counting only: m digits. Greedy's top
digit takes whatever bits are left, usually few, so its values crowd the lowest buckets. Pass 2
walks again and spreads the bits over the m digits: at a window start, with rho = bits still to
cover plus one for the borrow and k digits still to emit, the width is

    min(c + 1, max(ceil(rho / k) - 1, rho - (c + 1)(k - 1), 2))

(the second term keeps the rest coverable by k - 1 full windows; a single digit takes c + 1).

walk() states it on the running value, as one would on paper; walk_bits() is the form the kernel
runs: the half stays as it is, the walk keeps a bit position and a borrow, and the bits still to
cover follow from the half's bit length. The CPU test holds the two equal.

Digit d of scalar i goes to bucket (|d| - 1) / 2, entry code pos n_srs + i | sign << 31; bucket k
weighs 2 k + 1, so a commit is 2 sum (k + 1) B_k - sum B_k.
"""
from __future__ import annotations

import numpy as np

import msm_stage_ref as M

R = M.R
HALF = M.HALF
SIGN = M.SIGN
ROWS = 255  # bit positions 0 .. 254


def max_digits(c: int) -> int:
    return -(-255 // (c + 1))


def greedy_count(h: int, c: int) -> int:
    w, n = c + 1, 0
    while h:
        h >>= (h & -h).bit_length() - 1
        d = h & ((1 << w) - 1)
        if d >= 1 << (w - 1):
            d -= 1 << w
        h -= d
        n += 1
    return n


def width(rho: int, k: int, c: int) -> int:
    w = c + 1
    if k <= 1:
        return w
    return min(w, max(-(-rho // k) - 1, rho - w * (k - 1), 2))


def walk(h: int, c: int):
    """[(pos, d)] of the half h, on the running value."""
    out, pos, k = [], 0, greedy_count(h, c)
    while h:
        tz = (h & -h).bit_length() - 1
        h >>= tz
        pos += tz
        w = width(h.bit_length() + 1, k, c)
        d = h & ((1 << w) - 1)
        if d >= 1 << (w - 1):
            d -= 1 << w
        h -= d
        out.append((pos, d))
        k -= 1
    return out


def walk_bits(h: int, c: int):
    """The same pairs as the kernel finds them: position and borrow over the unchanged half."""
    L = h.bit_length()

    def run(emit):
        pos, carry, k, n = 0, 0, emit, 0
        while True:
            if not carry and pos >= L:
                return n
            while ((h >> pos) & 1) == carry:  # the next bit of the running value that is set
                pos += 1
            w = width(max(L - pos, 1) + 1, k, c) if emit else c + 1
            val = ((h >> pos) & ((1 << w) - 1)) + carry
            carry = 1 if val >= 1 << (w - 1) else 0
            if emit:
                out.append((pos, val - (carry << w)))
            pos += w
            k -= 1
            n += 1

    out = []
    m = run(0)
    if m:
        run(m)
    return out


def recode(s: int, c: int):
    """([(pos, d)], sign flip) of scalar s."""
    h, neg = M.scalar_half(s)
    return walk(h, c), neg


def entries_of(scalars, h: dict):
    """[(bucket, code)] of a slot's scalars under the snapshot header h (a part keeps its range)."""
    n, lo, B, c = h["n_srs"], h["b_lo"], h["B"], h["c"]
    out = []
    for i, s in enumerate(scalars):
        digits, neg = recode(s, c)
        for pos, d in digits:
            b = (abs(d) - 1) // 2 - lo
            if 0 <= b < B:
                out.append((b, (pos * n + i) | (SIGN if (d < 0) != neg else 0)))
    return out


def direct_dlog(h: dict, srs_dlog, scalars) -> int:
    """The slot's result by definition, a part's share of it for parts > 1."""
    if h["parts"] == 1:
        return sum(s * q for s, q in zip(scalars, srs_dlog)) % R
    n, tot = h["n_srs"], 0
    for b, code in entries_of(scalars, h):
        pos, i = divmod(code & 0x7FFFFFFF, n)
        v = srs_dlog[i] * pow(2, pos, R) * (2 * (b + h["b_lo"]) + 1)
        tot += -v if code & SIGN else v
    return tot % R


def bucket_counts(halves, c: int) -> np.ndarray:
    idx = [(abs(d) - 1) // 2 for h in halves for _, d in walk(h, c)]
    return np.bincount(np.asarray(idx, dtype=np.int64), minlength=1 << (c - 1))


def edge_halves(c: int) -> list:
    """0, 1, 2, 2^k and 2^k - 1 around k = c, c + 1, 253, 254, (r - 1) / 2 and its neighbours,
    alternating bits, long runs of ones and of zeros; every one clamped to a canonical half."""
    out = [0, 1, 2, 3, HALF, HALF - 1, HALF - 2]
    for k in (c - 1, c, c + 1, c + 2, 2 * c + 1, 2 * c + 2, 252, 253, 254):
        out += [1 << k, (1 << k) - 1, (1 << k) + 1]
    out += [int("10" * 127, 2), int("01" * 127, 2), int("1100" * 63, 2), int("0111" * 63, 2)]
    out += [(1 << 254) - (1 << 40), (1 << 200) + 1, ((1 << 100) - 1) << 77]
    out += [((1 << (c + 1)) - 1) << (c + 1), sum(1 << (k * (c + 1)) for k in range(max_digits(c)))]
    return [M._clamp(x) for x in out]


def edge_scalars(c: int) -> list:
    """Every edge half in both signs."""
    out = []
    for h in edge_halves(c):
        out += [h % R, (R - h) % R]
    return out
