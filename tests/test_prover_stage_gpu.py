"""The prover's quotient, permutation, public-input and coset-combine kernels (csrc/
prover_kernels.hip) stage by stage on edge operands, through plk_debug_prover_stage: the hook runs
the pk_* launcher the prover calls on the test's arrays, and every result is compared word for word
with the plain value reference of tests/prover_stage_ref.py (no tolerance anywhere).

Operands: every array draws independently per row from the pools of prover_stage_ref (0, 1, 2, 3,
r - 1, r - 2, (r +- 1) / 2, the values whose eight low 29-bit limbs are all 2^29 - 1, alternating
and single-max-limb rows, 2 000 random values; fixed seeds), plus rows whose operands are ALL the
same extreme. Nothing is skipped or filtered after generation: the only filter is "below r" where
the pools are built, and test_prover_stage_ref.py asserts the pools' sizes. Each test prints the
number of operand rows it ran (pytest -s)."""
from __future__ import annotations

import random

import numpy as np
import pytest

import prover_stage_ref as S
import pyref as P

pytestmark = pytest.mark.gpu
r = S.r
CH_KINDS = ("zero", "one", "minus_one", "random")
FLAG_SETS = {"none": 0, "range": 1, "logic": 2, "fixed": 4, "var": 8, "all": 15}


def challenges(kind, rng):
    names = ("alpha", "beta", "gamma", "range_sep", "logic_sep", "fixed_sep", "var_sep")
    fixed = {"zero": 0, "one": 1, "minus_one": r - 1}
    return {k: fixed[kind] if kind in fixed else rng.randrange(r) for k in names}


def quotient_case(n, seed, kind, has_pi):
    rng = random.Random(seed)
    blocks = 6 if n == 8 else 5
    nq = blocks * n
    col = lambda: S.draw(rng, nq)
    arr = {k: col() for k in ("a", "b", "c", "d", "z", "l1")}
    arr["pi"] = col() if has_pi else None
    arr["sel"] = [col() for _ in range(11)]
    arr["sigma"] = [col() for _ in range(4)]
    arr["elements"] = S.draw(rng, n)
    # the widget selectors: waves alternate between per-lane zero / non-zero, all zero and all
    # non-zero, so the rx_is_zero / fe_is_zero skips diverge inside a wave and between waves
    for q in (S.QRANGE, S.QLOGIC, S.QFIXED, S.QVAR):
        row = arr["sel"][q]
        for i in range(nq):
            mode = (i >> 6) % 3
            zero = (i & 1) == 0 if mode == 0 else mode == 1
            row[i] = 0 if zero else (row[i] or r - 1)
    for k, e in enumerate(S.extremes()):  # rows whose operands are all the same extreme
        i = (k % blocks) * n + 1 + k % (n - 2)  # never u = 0 or n - 1, which the wrap rows below own
        for key in ("a", "b", "c", "d", "z", "l1") + (("pi",) if has_pi else ()):
            arr[key][i] = e
        for row in arr["sel"] + arr["sigma"]:
            row[i] = e
        arr["elements"][i % n] = e
    # the last row of every block has every widget on, and the rows it could wrap to (u = 0 of its
    # own block: right; of the next block: wrong) differ in a, b, d and z
    for m in range(blocks):
        for q in (S.QRANGE, S.QLOGIC, S.QFIXED, S.QVAR):
            arr["sel"][q][m * n + n - 1] = arr["sel"][q][m * n + n - 1] or 1 + m
        for key in ("a", "b", "d", "z"):
            arr[key][m * n] = rng.randrange(r)
    for key in ("a", "b", "d", "z"):
        firsts = [arr[key][m * n] for m in range(blocks)]
        assert len(set(firsts)) == blocks
    ch = challenges(kind, rng)
    s_m = [rng.randrange(1, r) for _ in range(blocks)]
    vh_inv = [rng.randrange(1, r) for _ in range(blocks)]
    return blocks, arr, ch, s_m, vh_inv


def run_quotient(ctx, n, blocks, arr, ch, s_m, vh_inv, flag_bits):
    nq = blocks * n
    cat = lambda rows: [v for row in rows for v in row]
    arrays = [S.words_np(arr[k], -1) for k in "abcd"] + [
        S.words_np(arr["z"]), S.words_np(arr["pi"], 1) if arr["pi"] is not None else np.zeros((0, 4), np.uint64),
        S.words_np(arr["l1"]), S.words_np(cat(arr["sel"])), S.words_np(cat(arr["sigma"])),
        S.words_np(arr["elements"])]
    names = ("alpha", "beta", "gamma", "range_sep", "logic_sep", "fixed_sep", "var_sep")
    scalars = S.words_np([ch[k] for k in names] + s_m + vh_inv)
    return ctx.prover_stage("quotient", arrays, scalars, [n.bit_length() - 1, blocks, flag_bits], nq)


@pytest.mark.parametrize("flags", list(FLAG_SETS))
@pytest.mark.parametrize("n", (8, 16, 64, 512))
def test_quotient_rows_equal_the_row_formula(gpu_ctx, n, flags):
    """n = 8: 6 blocks, one partial workgroup; 16: 5 blocks; 64: 320 points, a ragged last
    workgroup; 512. flags none / range: k_quotient<true>; the others k_quotient<false> + _ext."""
    bits = FLAG_SETS[flags]
    fl = {"range": bool(bits & 1), "logic": bool(bits & 2), "fixed": bool(bits & 4), "var": bool(bits & 8)}
    rows = 0
    for has_pi in (True, False):
        for kind in CH_KINDS:
            blocks, arr, ch, s_m, vh_inv = quotient_case(n, 1000 * n + bits, kind, has_pi)
            got = run_quotient(gpu_ctx, n, blocks, arr, ch, s_m, vh_inv, bits)
            want = S.quotient(n, blocks, arr["a"], arr["b"], arr["c"], arr["d"], arr["z"], arr["pi"], arr["l1"],
                              arr["sel"], arr["sigma"], arr["elements"], ch, s_m, vh_inv, fl)
            bad = np.nonzero((got != S.words_np(want)).any(axis=1))[0]
            assert bad.size == 0, f"n={n} flags={flags} pi={has_pi} challenges={kind}: rows {bad[:8]} differ"
            rows += blocks * n
    print(f"quotient n={n} flags={flags}: {rows} operand rows")


def test_quotient_hook_refuses_bad_shapes(plk, gpu_ctx):
    blocks, arr, ch, s_m, vh_inv = quotient_case(8, 1, "random", True)
    with pytest.raises(plk.PlonkError) as e:  # a block count the prover never uses
        run_quotient(gpu_ctx, 8, 4, arr, ch, s_m[:4], vh_inv[:4], 0)
    assert e.value.status == plk.PLK_E_ARG
    arr["l1"] = arr["l1"][:-1]
    with pytest.raises(plk.PlonkError) as e:  # an array shorter than the domain
        run_quotient(gpu_ctx, 8, blocks, arr, ch, s_m, vh_inv, 0)
    assert e.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as e:
        gpu_ctx.prover_stage(99)
    assert e.value.status == plk.PLK_E_ARG
    with pytest.raises(plk.PlonkError) as e:
        gpu_ctx.prover_stage(-1)
    assert e.value.status == plk.PLK_E_ARG


@pytest.mark.parametrize("n", (1, 255, 256, 257))
def test_perm_numden_equals_its_definition(gpu_ctx, n):
    stride = n + 3  # the prover's wire columns are n + 3 apart
    rows = 0
    for kind in CH_KINDS:
        rng = random.Random(77 * n + CH_KINDS.index(kind))
        wires = [S.draw(rng, n) for _ in range(4)]
        sigmas = [S.draw(rng, n) for _ in range(4)]
        elements = S.draw(rng, n)
        for k, e in enumerate(S.extremes()[:n]):
            for row in wires + sigmas + [elements]:
                row[(3 * k + 1) % n] = e
        ch = challenges(kind, rng)
        pad = [rng.randrange(r) for _ in range(stride - n)]  # never read into the result
        flat = [v for w in wires for v in w + pad]
        got = gpu_ctx.prover_stage("perm_numden",
                                   [S.words_np(flat), S.words_np([v for s in sigmas for v in s]), S.words_np(elements)],
                                   S.words_np([ch["beta"], ch["gamma"], 7, 13, 17]), [n, stride], 2 * n)
        num, den = S.perm_numden(n, wires, sigmas, elements, ch["beta"], ch["gamma"])
        assert np.array_equal(got, S.words_np(num + den)), (n, kind)
        rows += n
    print(f"perm_numden n={n}: {rows} operand rows")


@pytest.mark.parametrize("n", (8, 64))
def test_pi_sparse_equals_the_rotated_l1_sum(plk, gpu_ctx, n):
    blocks = 6 if n == 8 else 5
    rng = random.Random(n)
    l1 = S.draw(rng, blocks * n)
    all_idx = [0, 6, n - 1, 3]
    for count in (1, 2, 3, 4):
        for vals in (S.draw(rng, count), [r - 1] * count, [0] * count):
            for idx in (all_idx[:count], all_idx[::-1][:count]):
                got = gpu_ctx.prover_stage("pi_sparse", [S.words_np(l1)], S.words_np(vals),
                                           [n.bit_length() - 1] + idx, blocks * n)
                want = S.pi_sparse(n, blocks, l1, idx, vals)
                assert np.array_equal(got, S.words_np(want, 1)), (n, count, idx)  # PI lands at exponent +1
    for count in (0, 5):
        with pytest.raises(plk.PlonkError) as e:
            gpu_ctx.prover_stage("pi_sparse", [S.words_np(l1)], S.words_np([1] * count),
                                 [n.bit_length() - 1] + [0] * count, blocks * n)
        assert e.value.status == plk.PLK_E_ARG


def test_pi_coef_equals_the_inverse_transform_of_a_sparse_vector(plk, gpu_ctx):
    k = 10
    n = 1 << k
    w_inv = pow(P.omega(k), -1, r)
    tw, x = [], 1
    for _ in range(n):
        tw.append(x)
        x = x * w_inv % r
    tw_np = S.words_np(tw, -1)  # the domain's inverse table is R'-domain
    n_inv = pow(n, -1, r)
    rng = random.Random(3)
    for count in (1, 5, 16):
        idx = [n - 1, 0, 6] + rng.sample(range(7, n - 1), 13)
        idx = idx[:count]
        for vals in (S.draw(rng, count), [r - 1] * count):
            got = gpu_ctx.prover_stage("pi_coef", [tw_np], S.words_np([v * n_inv % r for v in vals]), idx, n)
            assert np.array_equal(got, S.words_np(S.pi_coef(k, idx, vals))), count
    with pytest.raises(plk.PlonkError) as e:
        gpu_ctx.prover_stage("pi_coef", [tw_np], S.words_np([1] * 17), list(range(17)), n)
    assert e.value.status == plk.PLK_E_ARG


@pytest.mark.parametrize("n", (8, 257))
@pytest.mark.parametrize("blocks", (5, 6))
def test_coset_combine_equals_the_matrix_product(gpu_ctx, blocks, n):
    rng = random.Random(blocks * n)
    for trial in range(3):
        mat = [S.draw(rng, blocks, edge_share=1.0 if trial else 0.5) for _ in range(blocks)]
        vals = S.draw(rng, blocks * n)
        for k, e in enumerate(S.extremes()):
            for m in range(blocks):
                vals[m * n + k % n] = e
        if trial == 2:
            mat = [[r - 1] * blocks for _ in range(blocks)]
        got = gpu_ctx.prover_stage("coset_combine", [S.words_np(vals)],
                                   S.words_np([x for row in mat for x in row], -1), [blocks], blocks * n)
        assert np.array_equal(got, S.words_np(S.coset_combine(n, blocks, vals, mat))), (blocks, n, trial)


@pytest.mark.parametrize("blocks", (4, 7))
def test_coset_combine_refuses_other_block_counts(plk, gpu_ctx, blocks):
    with pytest.raises(plk.PlonkError) as e:
        gpu_ctx.prover_stage("coset_combine", [S.words_np([1] * (blocks * 8))],
                             S.words_np([1] * (blocks * blocks)), [blocks], blocks * 8)
    assert e.value.status == plk.PLK_E_ARG
