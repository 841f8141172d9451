"""The lazy butterfly arithmetic of the NTT pass kernel (csrc/ntt.hip) pinned at its bounds.

CPU part: the Python-integer model (tests/ntt_lazy_ref.py) runs every helper over operand sets
that sit on the edges of the documented input ranges and asserts, step by step, what the device
code relies on (no 32-bit limb wraps, reduce_q's table index below kQMax and its result exactly
value - q r >= 0, product columns below 2^64, rx_mul's operand contract), that every helper's
output meets the precondition written at its consumer (the induction that makes a per-step test
cover a whole pass), and that each output's residue is the butterfly's mathematical value.

GPU part: plk_debug_ntt_lazy_op runs the very functions k_ntt_pass calls on the same rows, and
every output must equal the model limb for limb (the stores: word for word).

No case is filtered out: a generated row that misses the precondition of the op it is fed to is
an assertion failure of the generator, and the share of skipped cases is asserted to be 0."""
import functools

import numpy as np
import pytest

import ntt_lazy_ref as Z

F, r = Z.F, Z.r
OPS = ("reduce_q", "add_u", "sub_u", "sub_u2_11", "r4", "r4_h1", "r2first", "odd_last",
       "store0", "store1", "store2")
KINDS = ("edges", "random")
# bounds written at the helpers in ntt.hip (in units of r): outputs of r4_math, of the odd
# stages and of the store's reduce_q
DOC_BOUND = {"r4": 4, "r4_h1": 4, "r2first": (1.6, 2), "odd_last": 5}


@functools.lru_cache(maxsize=None)
def generated(op: str, kind: str) -> tuple:
    """The cases of one op as tuples of operand rows, straight from the generators."""
    if op == "reduce_q":
        return tuple((row,) for row in Z.reduce_q_rows(kind))
    if op == "add_u":  # normalised pairs below 5r, and the sums of sums o0 takes (y0 + y1)
        pairs = [(a, b) for a, b, _ in Z.pair_cases(5, kind)]
        return tuple(dict.fromkeys(pairs + list(Z.sub_u2_cases(kind))))
    if op == "sub_u":
        return tuple(dict.fromkeys((a, b) for a, b, _ in Z.pair_cases(2, kind)))
    if op == "sub_u2_11":
        return Z.sub_u2_cases(kind)
    if op == "r4":
        return tuple(x + tw for x, tw in Z.r4_cases(kind))
    if op == "r4_h1":
        return tuple(x + tw[:1] for x, tw in Z.r4_cases(kind))
    if op == "r2first":
        return Z.pair_cases(2, kind)
    if op == "odd_last":
        return tuple(dict.fromkeys((a, c) for a, c, _ in Z.pair_cases(5, kind)))
    rows = Z.store_rows(kind)
    if op == "store0":
        return tuple((v,) for v in rows)
    s = Z.scale_words()
    if kind == "edges":
        return tuple((v, w) for w in s for v in rows)
    rnd = [Z.words_of(F.value(t)) for t in Z.random_twiddles(len(rows), 90)]
    if op == "store1":  # a kernel argument, one launch per scale: three random scales
        rnd = rnd[:3]
    return tuple((v, rnd[i % len(rnd)]) for i, v in enumerate(rows))


def check_preconditions(op: str, case):
    """The documented precondition of the op, on one generated case."""
    if op == "reduce_q":
        Z.check_reduce_q_input(case[0])
    elif op == "add_u":
        for row in case:
            Z.check_sum_operand(row)
    elif op in ("sub_u", "r2first"):
        Z.check_normalised_below(case[0], 2, op)
        Z.check_normalised_below(case[1], 2, op)
        if op == "r2first":
            Z.check_twiddle(case[2])
    elif op == "sub_u2_11":
        Z.check_sum_operand(case[0])
        Z.check_sum_operand(case[1])
    elif op in ("r4", "r4_h1"):
        for row in case[:4]:
            Z.check_normalised_below(row, 5, op)
        for row in case[4:]:
            Z.check_twiddle(row)
    elif op == "odd_last":
        Z.check_normalised_below(case[0], 5, op)
        Z.check_normalised_below(case[1], 5, op)
    else:
        Z.check_normalised_below(case[0], 5, op)
        if op != "store0":
            assert case[1][8] == 0
            Z.check_twiddle(Z.unpack_words(case[1]))


def run_model(M, op: str, case) -> tuple:
    if op == "reduce_q":
        return (M.reduce_q(case[0]),)
    if op == "add_u":
        return (M.add_u(*case),)
    if op == "sub_u":
        return (M.sub_u(*case),)
    if op == "sub_u2_11":
        return (M.sub_u2(case[0], case[1], M.cp["r4_y01"]),)
    if op == "r4":
        return M.r4_math(False, case[:4], case[4:])
    if op == "r4_h1":
        return M.r4_math(True, case[:4], case[4:])
    if op == "r2first":
        return M.r2first(*case)
    if op == "odd_last":
        return M.odd_last(*case)
    if op == "store0":
        return (M.store0(case[0]),)
    return (M.store_scaled(case[0], case[1]),)


def check_consumer(op: str, out):
    """Every output against the precondition written where ntt.hip consumes it."""
    if op == "add_u":  # o0 = reduce_q(add_u(y0, y1)), and the sums that sub_u2 subtracts
        Z.check_reduce_q_input(out[0])
    elif op == "sub_u":  # a multiplicand: limbs below 2^29 + 2^30, value in (r, 5r)
        assert max(out[0]) < (1 << 29) + (1 << 30) and r < F.value(out[0]) < 5 * r
        Z.check_mul_operands(out[0], F.limbs(r - 1))
    elif op == "sub_u2_11":  # feeds reduce_q (h == 1) and rx_mul: limbs below 2^31.6, (r, 21r)
        Z.check_reduce_q_input(out[0])
        assert r < F.value(out[0]) < 21 * r
        Z.check_mul_operands(out[0], F.limbs(r - 1))
    elif op in ("r4", "r4_h1", "r2first", "odd_last"):  # the next stage, then the store
        for row in out:
            Z.check_normalised_below(row, 5, f"{op} output")
    elif op == "reduce_q":
        assert F.normalised(out[0])


@functools.lru_cache(maxsize=None)
def expected(op: str, kind: str):
    """(cases, model outputs, skipped): computed once, shared by the CPU and the GPU tests."""
    M = Z.Model()
    cases = generated(op, kind)
    outs = []
    for case in cases:
        check_preconditions(op, case)  # an assertion, never a filter
        out = run_model(M, op, case)
        check_consumer(op, out)
        outs.append(out)
    # skipped = generated - run. Nothing above can drop a case, so this is 0 by construction:
    # the figure is kept so that a filter added later shows up in the tests that assert it
    return cases, tuple(outs), len(generated(op, kind)) - len(outs), M


def inv_tw(row) -> int:
    """The plain value a table row multiplies by: w / R' mod r."""
    return F.value(row) * Z.RP_INV % r


# ------------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
def test_model_bounds_and_induction(op, kind):
    """The model's own assertions over the operand sets (Model(strict=True) raises on a wrapped
    limb, a table index >= kQMax, an inexact reduce_q, a column >= 2^64 or a product operand
    outside rx_mul's contract), every output inside its consumer's precondition, no case
    skipped, and the tighter output bounds written in ntt.hip's comments."""
    cases, outs, skipped, M = expected(op, kind)
    assert len(cases) >= (2000 if kind == "random" else 30), len(cases)
    assert skipped == 0 and len(outs) == len(cases)
    assert all(q < Z.K_QMAX for q in M.q_seen)
    assert M.max_limb < 1 << 32 and M.max_column < 1 << 64
    if op in DOC_BOUND:
        b = DOC_BOUND[op]
        for out in outs:
            for j, row in enumerate(out):
                assert F.value(row) < (b[j] if isinstance(b, tuple) else b) * r, (op, j, row)
    if op == "store0":  # "< 1.6r" at the store's reduce_q
        assert all(F.value(Z.Model().reduce_q(c[0])) < 1.6 * r for c in cases)
    if op.startswith("store"):
        for out in outs:
            assert F.value(Z.unpack_words(out[0])) < r and out[0][8] == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
def test_model_agrees_with_modular_arithmetic(op, kind):
    """Each output's residue is the operation's mathematical value mod r."""
    cases, outs, _, _ = expected(op, kind)
    res = Z.residue
    for case, out in zip(cases, outs):
        if op == "reduce_q":
            want = [res(case[0])]
        elif op == "add_u":
            want = [res(case[0]) + res(case[1])]
        elif op in ("sub_u", "sub_u2_11"):
            want = [res(case[0]) - res(case[1])]
            c = 3 if op == "sub_u" else 11
            assert F.value(out[0]) == F.value(case[0]) + c * r - F.value(case[1])
        elif op in ("r4", "r4_h1"):
            x0, x1, x2, x3 = (res(v) for v in case[:4])
            if op == "r4":
                wa, wb, wc = (inv_tw(t) for t in case[4:])
                y2, y3 = (x0 - x2) * wa, (x1 - x3) * wb
                want = [x0 + x1 + x2 + x3, (x0 + x2 - x1 - x3) * wc, y2 + y3, (y2 - y3) * wc]
            else:
                y2, y3 = x0 - x2, (x1 - x3) * inv_tw(case[4])
                want = [x0 + x1 + x2 + x3, x0 + x2 - x1 - x3, y2 + y3, y2 - y3]
        elif op == "r2first":
            a, v = res(case[0]), res(case[1])
            want = [a + v, (a - v) * inv_tw(case[2])]
        elif op == "odd_last":
            a, c = res(case[0]), res(case[1])
            want = [a + c, a - c]
        else:
            s = 1 if op == "store0" else inv_tw(Z.unpack_words(case[1]))
            want = [res(case[0]) * s]
            assert F.value(Z.unpack_words(out[0])) == want[0] % r  # canonical: the value itself
            continue
        assert [res(row) for row in out] == [w % r for w in want], (op, case)


def test_operand_classes():
    """The operand sets hold the extremes they are meant to."""
    top5, top2 = F.top_of(5 * r - 1), F.top_of(2 * r - 1)
    d5, d2 = Z.data_rows(5), Z.data_rows(2)
    assert {0, 1, r - 1, r, r + 1, 2 * r - 1, 2 * r, 4 * r - 1, 5 * r - 1} <= {F.value(v) for v in d5}
    assert {0, 1, r - 1, r, r + 1, 2 * r - 1} <= {F.value(v) for v in d2} and max(F.value(v) for v in d2) < 2 * r
    for rows, top in ((d5, top5), (d2, top2)):
        assert Z.max_limb_row(0) in rows and Z.max_limb_row(top - 1) in rows
        assert set(Z.alternating_rows(top - 1)) <= set(rows)
    assert len(d5) == 13
    # the fourfold cross: every row in every position, under distinct and equal twiddles
    cases = generated("r4", "edges")
    assert len(cases) == 13 ** 4 + 81 * 15
    for k in range(4):
        assert {c[k] for c in cases} == set(d5)
    tw = Z.twiddle_rows()
    assert {F.value(t) for t in tw} >= {0, 1, F.one, r - 1} and Z.max_limb_row(F.top_of(r - 1) - 1) in tw
    assert sum(1 for c in cases if len(set(c[4:])) == 3) > len(cases) // 2
    for k in range(4, 7):
        assert {c[k] for c in cases} == set(tw)
    hi = F.limbs(5 * r - 1)
    assert {c[4:] for c in cases if c[:4] == (hi,) * 4} == set(Z.twiddle_triples())
    # reduce_q: every q from both limb extremes, the multiples of r and of 2^255
    rq = [c[0] for c in generated("reduce_q", "edges")]
    vals = {F.value(v) for v in rq if F.normalised(v)}
    for q in range(Z.K_QMAX):
        assert (0,) * 8 + (q << Z.Q_SHIFT,) in rq and ((1 << 31) - 1,) * 8 + (q << Z.Q_SHIFT,) in rq
        assert {q * r, q * r + 1, ((q + 1) << 255) - 1, q << 255} <= vals and (q == 0 or q * r - 1 in vals)
    _, _, _, M = expected("reduce_q", "edges")
    assert set(M.q_seen) == set(range(Z.K_QMAX))
    # the lazy differences reach their limb and value bounds
    subs = [F.value(o[0]) for o in expected("sub_u2_11", "edges")[1]]
    assert min(subs) == r + 2 and max(subs) > 20 * r
    assert max(max(o[0]) for o in expected("sub_u2_11", "edges")[1]) >= 1 << 31
    # the stores see the values fe_reduce_once must get right: r itself, r - 1, 0, 2r - 1
    st = {F.value(Z.Model().reduce_q(c[0])) for c in generated("store0", "edges")}
    assert {0, 1, r - 1, r, r + 1} <= st
    outs = {F.value(Z.unpack_words(o[0])) for o in expected("store0", "edges")[1]}
    assert {0, 1, r - 1} <= outs and max(outs) == r - 1


def test_model_rejects_a_wrong_table_row_and_a_low_multiple():
    """The model is not vacuous: a kZTab row replaced by its lower neighbour's (correct mod r,
    one r too large) breaks reduce_q's exactness, and a multiple of r lowered by one in a lazy
    subtraction of r4_math (rx_sub_u<5> for <6>, sub_u2<10> for <11>) wraps a limb for operands
    at the top of the input range only."""
    zt = list(Z.make_ztab())
    zt[25] = zt[24]
    M = Z.Model(ztab=tuple(zt))
    with pytest.raises(AssertionError):
        M.reduce_q((0,) * 8 + (25 << Z.Q_SHIFT,))
    M = Z.Model(cp={"r4_x13": 5})
    tw = Z.twiddle_rows()
    ok = (F.limbs(1), F.limbs(r), F.limbs(2 * r), F.limbs(4 * r - 1))
    M.r4_math(True, ok, tw[:1])
    with pytest.raises(AssertionError):
        M.r4_math(True, (ok[0], F.limbs(1), ok[2], F.limbs(5 * r - 1)), tw[:1])
    M = Z.Model(cp={"r4_y01": 10})  # sub_u2<10>: the top limb wraps under the largest y1 only
    M.r4_math(False, ok, tw[:3])
    with pytest.raises(AssertionError):
        M.r4_math(False, (F.limbs(0), F.limbs(5 * r - 1), F.limbs(0), F.limbs(5 * r - 1)), tw[:3])


def test_wrapping_model_equals_the_strict_one_inside_the_contract():
    """Model(strict=False) (registers that wrap, rx_mul as its 64-bit column algorithm: the form
    a changed constant is studied with) gives the strict model's limbs wherever every bound
    holds, and mul_columns is the exact Montgomery value there."""
    W = Z.Model(strict=False)
    for op in ("r4", "r4_h1", "r2first", "odd_last", "store0", "store2"):
        cases, outs, _ = expected(op, "random")[:3]
        for case, out in list(zip(cases, outs))[:200]:
            assert run_model(W, op, case) == out, (op, case)
    a, b = Z.sub_u2_cases("edges")[-1]
    for w in Z.twiddle_rows():
        d = Z.Model().sub_u2(a, b)
        assert Z.mul_columns(d, w) == F.limbs(F.mont(F.value(d) * F.value(w)))
    assert max(W.q_seen) < Z.K_QMAX
    # outside it the wrapping model reports the index instead of asserting
    assert Z.Model(strict=False).reduce_q((0,) * 8 + (Z.K_QMAX << Z.Q_SHIFT,)) is None


# ------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
def test_hook_rejects_null_arrays_and_unknown_ops(plk, gpu_ctx):
    """With a live context: a NULL input or output array and an unknown op code are PLK_E_ARG
    (the call without a context is refused in tests/test_rx_gpu.py, with the other hooks)."""
    import ctypes
    lib = plk.plonk._lib()
    row = np.zeros(9, dtype=np.uint32)
    p = row.ctypes.data_as(ctypes.c_void_p)
    assert lib.plk_debug_ntt_lazy_op(gpu_ctx.handle, 0, None, p, 1) == plk.PLK_E_ARG
    assert lib.plk_debug_ntt_lazy_op(gpu_ctx.handle, 0, p, None, 1) == plk.PLK_E_ARG
    assert lib.plk_debug_ntt_lazy_op(gpu_ctx.handle, 11, p, p, 1) == plk.PLK_E_ARG
    assert lib.plk_debug_ntt_lazy_op(gpu_ctx.handle, -1, p, p, 1) == plk.PLK_E_ARG
    assert lib.plk_debug_ntt_lazy_op(gpu_ctx.handle, 0, p, p, 0) == plk.PLK_OK


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", OPS)
def test_hook_equals_model(gpu_ctx, op, kind):
    """Every output of plk_debug_ntt_lazy_op equals the model limb for limb (the stores: the
    packed canonical word, word for word)."""
    cases, outs, skipped, _ = expected(op, kind)
    assert skipped == 0
    cols = [np.array([c[k] for c in cases], dtype=np.uint32) for k in range(len(cases[0]))]
    want = np.array(outs, dtype=np.uint32)
    if op == "store1":  # the scale is a kernel argument: one call per scale
        got = np.zeros_like(want)
        keys = cols[1].view([("", cols[1].dtype)] * 9).ravel()
        scales = np.unique(keys)
        assert 3 <= len(scales) <= 5
        done = np.zeros(len(cases), dtype=bool)
        for k in scales:
            idx = np.flatnonzero(keys == k)
            got[idx] = gpu_ctx.ntt_lazy_op(op, cols[0][idx], cols[1][idx])
            done[idx] = True
        assert done.all()
    else:
        got = gpu_ctx.ntt_lazy_op(op, *cols)
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert bad.size == 0, (f"{op} {kind}: {bad.size} of {len(cases)} cases differ; first: operands "
                           f"{cases[bad[0]]} gave {got[bad[0]].tolist()}, expected {want[bad[0]].tolist()}")
