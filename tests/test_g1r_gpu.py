"""The XYZZ group law of the MSM's device stages (csrc/g1r.hpp) through plk_debug_g1r_op, against
oracle/pyref.py: every addition form (the four straight-line mixed additions of k_accumulate with
their repair-after sequence, g1r_madd_lazy, g1r_add_lazy, the quad-cooperative g1r_add_quad, the
doublings, the non-lazy forms) on operands whose coordinates sit at the bottom and at the top of
their documented ranges (X in [0, 8p), Y in [0, 4p), ZZ, ZZZ in [0, 2p)), in the generic case and
in every exceptional one: doubling, inverse, either operand at infinity (ZZ = 0 and ZZ = p), with
and without the lazy negation 4p - y."""
import functools
import random

import numpy as np
import pytest

import pyref as P
import rx_ref as R

F = R.FP
p = F.p
LAZY, PLAIN = (8, 4, 2, 2), (2, 2, 2, 2)  # the coordinates' ranges, in multiples of p
MIXED_LAZY = ("madd_000", "madd_100", "madd_110", "madd_111", "madd_lazy")
# op -> (q is affine, the operands' ranges, the result's ranges)
BINARY_OPS = {**{op: (True, LAZY, LAZY) for op in MIXED_LAZY},
              "add_affine": (True, PLAIN, PLAIN),
              "add_lazy": (False, LAZY, LAZY), "add_quad": (False, LAZY, LAZY),
              "add": (False, PLAIN, PLAIN)}
N_POINTS = 40


@functools.lru_cache(maxsize=None)
def points() -> tuple:
    pts = [P.G1_GEN]
    while len(pts) < N_POINTS:
        pts.append(P.g1_add(pts[-1], P.G1_GEN))
    return tuple(pts)


def affine_row(pt, lifts=(0, 0)) -> tuple:
    """An affine operand: X, Y in [0, 2p); the ZZ, ZZZ rows are not read (filled with ones)."""
    x, y = pt
    one = F.limbs(F.one)
    return (F.limbs(x * F.Rp % p + lifts[0] * p), F.limbs(y * F.Rp % p + lifts[1] * p), one, one)


def infinity_row(rng, ranges, zz: int) -> tuple:
    """Infinity as ZZ = 0 or ZZ = p under arbitrary non-zero in-range X, Y, ZZZ."""
    return (F.limbs(rng.randrange(1, ranges[0] * p)), F.limbs(rng.randrange(1, ranges[1] * p)),
            F.limbs(zz), F.limbs(rng.randrange(1, ranges[3] * p)))


@functools.lru_cache(maxsize=None)
def binary_cases(affine_q: bool, ranges: tuple) -> tuple:
    """(class, P, Q, flag, p row, q row): P + (-1)^flag Q is the expected sum (None: infinity).
    Every class comes with the coordinates of both operands at the bottom of their ranges, at the
    top, and mixed."""
    rng = random.Random(1000 * affine_q + sum(ranges))
    pts = points()
    top = tuple(k - 1 for k in ranges)
    lifts = [((0, 0, 0, 0), (0, 0, 0, 0)), (top, top), ((0, top[1], top[2], 0), (top[0], 0, 0, top[3])),
             ((top[0], 0, 0, top[3]), (0, top[1], top[2], 0))]
    out = []

    def xyzz(pt, lift):
        return R.xyzz_row(pt, rng.randrange(2, p), lift)

    def q_row(pt, lift):
        return affine_row(pt, (min(lift[0], 1), min(lift[1], 1))) if affine_q else xyzz(pt, lift)

    for i, pt in enumerate(pts):
        lp, lq = lifts[i % len(lifts)]
        other = pts[(7 * i + 3) % N_POINTS]
        assert other != pt and other != P.g1_neg(pt)
        neg = P.g1_neg(pt)
        for flag in (0, 1):
            out.append(("generic", pt, other, flag, xyzz(pt, lp), q_row(other, lq)))
            # q = p up to the sign the flag undoes: p under another z and other lifts than q
            out.append(("double", pt, neg if flag else pt, flag, xyzz(pt, lp), q_row(neg if flag else pt, lq)))
            out.append(("inverse", pt, pt if flag else neg, flag, xyzz(pt, lp), q_row(pt if flag else neg, lq)))
            for zz in (0, p):
                out.append(("p_inf", None, other, flag, infinity_row(rng, ranges, zz), q_row(other, lq)))
                if not affine_q:
                    out.append(("q_inf", pt, None, flag, xyzz(pt, lp), infinity_row(rng, ranges, zz)))
                    out.append(("both_inf", None, None, flag, infinity_row(rng, ranges, p - zz),
                                infinity_row(rng, ranges, zz)))
    return tuple(out)


def expected_sum(case):
    _, a, b, flag, _, _ = case
    return P.g1_add(a, P.g1_neg(b) if flag else b)


def check_rows(rows, expected, ranges, what):
    """Normalised limbs, coordinates inside the ranges the next addition assumes, the affine
    point (infinity: ZZ in {0, p}), ZZ^3 == ZZZ^2."""
    for i, (row, exp) in enumerate(zip(rows, expected)):
        for c, k in zip(row, ranges):
            assert F.normalised(c) and 0 <= F.value(c) < k * p, (what, i, c)
        got, consistent = R.xyzz_decode(row)
        assert got == exp, (what, i)
        assert consistent, (what, i)


# ------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("affine_q,ranges", [(True, LAZY), (True, PLAIN), (False, LAZY), (False, PLAIN)])
def test_case_generator(affine_q, ranges):
    cases = binary_cases(affine_q, ranges)
    classes = {c[0] for c in cases}
    assert classes == {"generic", "double", "inverse", "p_inf"} | (set() if affine_q else {"q_inf", "both_inf"})
    hit_top = [False] * 4
    hit_bottom = [False] * 4
    for cls, a, b, flag, prow, qrow in cases:
        assert P.g1_is_on_curve(a) and P.g1_is_on_curve(b)
        for row, pt, rg in ((prow, a, ranges), (qrow, b, (2, 2, 2, 2) if affine_q else ranges)):
            assert all(F.normalised(c) and F.value(c) < k * p for c, k in zip(row, rg))
            if pt is None:
                assert F.value(row[2]) in (0, p)
            elif row is prow or not affine_q:
                assert R.xyzz_decode(row) == (pt, True)
                for j in range(4):
                    hit_top[j] |= F.value(row[j]) >= (rg[j] - 1) * p
                    hit_bottom[j] |= F.value(row[j]) < p
            else:
                rinv = pow(F.Rp, -1, p)
                assert (F.value(row[0]) * rinv % p, F.value(row[1]) * rinv % p) == pt
        if cls == "double":
            assert expected_sum((cls, a, b, flag, prow, qrow)) == P.jac_to_affine(
                P.jac_double(P.jac_from_affine(a)))
            assert prow != qrow
        if cls == "inverse":
            assert expected_sum((cls, a, b, flag, prow, qrow)) is None
    assert all(hit_top) and all(hit_bottom)
    assert {c[3] for c in cases if c[0] == "double"} == {0, 1}
    assert {F.value(c[4][2]) for c in cases if c[0] == "p_inf"} == {0, p}


# ------------------------------------------------------------------------------- GPU tests
def as_np(rows) -> np.ndarray:
    return np.array(rows, dtype=np.uint32)


def run_binary(ctx, op, prow, qrow, flags):
    """The device rows of one binary op; for add_quad the four lanes must agree limb for limb and
    lane 0 is returned."""
    out = ctx.g1r_op(op, as_np(prow), as_np(qrow), np.array(flags, dtype=np.uint32))
    if op == "add_quad":
        assert (out == out[:, :1]).all(), "the lanes of a quad disagree"
        out = out[:, 0]
    return out.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(BINARY_OPS))
def test_additions(gpu_ctx, op):
    affine_q, ranges, out_ranges = BINARY_OPS[op]
    cases = binary_cases(affine_q, ranges)
    out = run_binary(gpu_ctx, op, [c[4] for c in cases], [c[5] for c in cases], [c[3] for c in cases])
    for cls in sorted({c[0] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c[0] == cls]
        check_rows([out[i] for i in idx], [expected_sum(cases[i]) for i in idx], out_ranges,
                   f"{op} {cls}")


@pytest.mark.gpu
def test_doublings_and_finish(gpu_ctx):
    rng = random.Random(5)
    pts = points()
    dbl = [P.jac_to_affine(P.jac_double(P.jac_from_affine(pt))) for pt in pts]
    for op, ranges, out_ranges in (("dbl_lazy", LAZY, (8, 2, 2, 2)), ("dbl", PLAIN, PLAIN),
                                   ("lazy_finish", LAZY, PLAIN)):
        top = tuple(k - 1 for k in ranges)
        rows, exp = [], []
        for i, pt in enumerate(pts):
            for lift in ((0, 0, 0, 0), top, (top[0], 0, top[2], 0), (0, top[1], 0, top[3])):
                rows.append(R.xyzz_row(pt, rng.randrange(2, p), lift))
                exp.append(pt if op == "lazy_finish" else dbl[i])
        for zz in (0, p):
            rows.append(infinity_row(rng, ranges, zz))
            exp.append(None)
        out = gpu_ctx.g1r_op(op, as_np(rows)).tolist()
        check_rows(out, exp, out_ranges, op)
        if op == "dbl_lazy":  # X3 = M^2 + 6p - 2S in (2p, 8p)
            assert all(F.value(r[0]) > 2 * p for r, e in zip(out, exp) if e is not None)
        if op == "lazy_finish":  # ZZ, ZZZ untouched
            assert all(o[2:] == [list(c) for c in r[2:]] for o, r in zip(out, rows))
    rows = [affine_row(pt, (i % 2, (i // 2) % 2)) for i, pt in enumerate(pts)]
    out = gpu_ctx.g1r_op("dbl_affine", as_np(rows)).tolist()
    check_rows(out, dbl, PLAIN, "dbl_affine")


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(BINARY_OPS))
def test_accumulator_chains(gpu_ctx, op):
    """64 additions into one accumulator, each result fed back raw: of the same point (the first
    addition is a doubling) and of alternating -+G from both phases (through infinity and back:
    the tau = +-1 case of test_msm_repeated_points, form by form)."""
    affine_q, ranges, out_ranges = BINARY_OPS[op]
    rng = random.Random(9)
    pts = points()
    G = pts[0]
    bases = [G, pts[4], pts[11]]
    chains = [(b, lambda k: 0) for b in bases] + [(G, lambda k: (k + 1) % 2), (G, lambda k: k % 2)]
    acc = [R.xyzz_row(b, 1, (0, 0, 0, 0)) for b, _ in chains]
    q = [affine_row(b) if affine_q else R.xyzz_row(b, rng.randrange(2, p), (0, 0, 0, 0)) for b, _ in chains]
    exp = [b for b, _ in chains]
    for k in range(64):
        flags = [f(k) for _, f in chains]
        exp = [P.g1_add(e, P.g1_neg(b) if fl else b) for e, (b, _), fl in zip(exp, chains, flags)]
        acc = run_binary(gpu_ctx, op, acc, q, flags)
        check_rows(acc, exp, out_ranges, f"{op} step {k}")
    assert exp[0] == P.g1_mul(G, 65) and exp[3] in (None, G) and exp[4] in (G, pts[1])
