"""CPU tests of tests/prover_stage_ref.py: the bound propagation of every modelled chain of
csrc/prover_kernels.hip passes from the input contract alone, the limb-exact model computes the
stage definitions (the value reference) on the edge-operand sets of the GPU tests, and the model
rejects deliberately weakened chains."""
from __future__ import annotations

import random

import pytest

import prover_stage_ref as S

r, F = S.r, S.F
CH_KINDS = ("zero", "one", "minus_one", "random")


def challenges(kind: str, rng: random.Random) -> dict:
    names = ("alpha", "beta", "gamma", "range_sep", "logic_sep", "fixed_sep", "var_sep")
    fixed = {"zero": 0, "one": 1, "minus_one": r - 1}
    return {k: fixed[kind] if kind in fixed else rng.randrange(r) for k in names}


def test_pools_have_the_stated_sizes_and_stay_below_r():
    p = S.canonical_pools()
    assert {k: len(v) for k, v in p.items()} == {"small": 8, "max_low": 66, "edges": len(p["edges"]),
                                                 "alt": 2, "single": 8, "random": 2000}
    assert len(p["edges"]) >= 20
    assert all(0 <= v < r for vs in p.values() for v in vs)
    assert all(F.limbs(v)[:-1] == (S.MASK,) * 8 for v in p["max_low"])
    assert S.max_low_value(S.MAX_LOW_TOPS - 1) < r <= S.MAX_LOW + (S.MAX_LOW_TOPS << S.TOP_SHIFT)
    assert {0, 1, 2, 3, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2} == set(p["small"])
    assert len(S.pool_values()) == sum(len(v) for v in p.values())


def test_bound_propagation_passes_for_every_chain():
    got = S.propagate_all()
    assert set(got) == {"k_quotient<true>", "k_quotient<false>", "k_perm_numden", "k_coset_combine<5>",
                        "k_coset_combine<6>", "k_pi_sparse", "k_lincomb", "k_eval_partial"}
    for name, d in got.items():
        assert d["max_column_bits"] <= 64 and d["max_limb_bits"] <= 32, (name, d)
    # the figures the kernels' comments state: the carry-free sums' limbs stay below 2^31, the
    # largest product is 16 r^2 (canonical inputs: the add3_u factors are below 4r, not 6r)
    assert got["k_quotient<true>"]["max_limb_bits"] == 31
    assert got["k_quotient<true>"]["max_product_r2"] == pytest.approx(16.0)
    assert got["k_perm_numden"]["max_product_r2"] == pytest.approx(16.0)
    # and with the range widget and PI off (the other code path)
    S.chain_quotient(S.Bounds(), None, None, has_range=False, has_pi=False)


def quotient_case(n, seed, kind, has_pi=True):
    """Plain arrays for one small quotient domain with edge operands, as the GPU test builds them."""
    rng = random.Random(seed)
    blocks = 6 if n == 8 else 5
    nq = blocks * n
    col = lambda: S.draw(rng, nq)
    arr = {k: col() for k in ("a", "b", "c", "d", "z", "l1")}
    arr["pi"] = col() if has_pi else None
    arr["sel"] = [col() for _ in range(11)]
    arr["sigma"] = [col() for _ in range(4)]
    arr["elements"] = S.draw(rng, n)
    for k, e in enumerate(S.extremes()):  # rows whose operands are all the same extreme
        i = (5 * k + 2) % nq
        for key in ("a", "b", "c", "d", "z", "l1") + (("pi",) if has_pi else ()):
            arr[key][i] = e
        for row in arr["sel"] + arr["sigma"]:
            row[i] = e
        arr["elements"][i % n] = e
    ch = challenges(kind, rng)
    s_m = [rng.randrange(1, r) for _ in range(blocks)]
    vh_inv = [rng.randrange(1, r) for _ in range(blocks)]
    return blocks, arr, ch, s_m, vh_inv


@pytest.mark.parametrize("kind", CH_KINDS)
@pytest.mark.parametrize("final", (True, False))
def test_concrete_quotient_model_equals_the_value_reference(kind, final):
    n = 8
    blocks, arr, ch, s_m, vh_inv = quotient_case(n, 11, kind)
    flags = {"range": True, "logic": False, "fixed": False, "var": False}
    want = S.quotient(n, blocks, arr["a"], arr["b"], arr["c"], arr["d"], arr["z"], arr["pi"], arr["l1"],
                      arr["sel"], arr["sigma"], arr["elements"], ch, s_m,
                      vh_inv if final else [1] * blocks, flags)
    K = S.quotient_constant_words(ch, s_m, vh_inv)
    A = S.Concrete()
    for i in range(blocks * n):
        m, u = divmod(i, n)
        nx = m * n + (u + 1) % n
        w = {k: S.word(arr[k][i], -1) for k in "abcd"}
        w.update(z=S.word(arr["z"][i]), z_next=S.word(arr["z"][nx]), d_next=S.word(arr["d"][nx], -1),
                 pi=S.word(arr["pi"][i], 1), l1=S.word(arr["l1"][i]), element=S.word(arr["elements"][u]),
                 sel=[S.word(row[i]) for row in arr["sel"]], sigma=[S.word(row[i]) for row in arr["sigma"]])
        got = S.chain_quotient(A, w, K, blk=m, final=final)
        assert got == S.word(want[i], 0 if final else 1), (i, kind)
    assert A.max_column < 1 << 64 and A.max_limb < 1 << 31


@pytest.mark.parametrize("kind", CH_KINDS)
def test_concrete_perm_numden_model_equals_the_value_reference(kind):
    rng = random.Random(5)
    n = 96
    wires = [S.draw(rng, n) for _ in range(4)]
    sigmas = [S.draw(rng, n) for _ in range(4)]
    elements = S.draw(rng, n)
    for k, e in enumerate(S.extremes()):
        for row in wires + sigmas + [elements]:
            row[k] = e
    ch = challenges(kind, rng)
    num, den = S.perm_numden(n, wires, sigmas, elements, ch["beta"], ch["gamma"])
    K = S.perm_constant_words(ch["beta"], ch["gamma"])
    A = S.Concrete()
    for i in range(n):
        w = {"wires": [S.word(c[i]) for c in wires], "sigmas": [S.word(c[i]) for c in sigmas],
             "element": S.word(elements[i])}
        assert S.chain_perm_numden(A, w, K) == (S.word(num[i]), S.word(den[i]))


def test_concrete_small_chains_equal_the_value_reference():
    rng = random.Random(9)
    A = S.Concrete()
    for blocks in (5, 6):
        mat = [S.draw(rng, blocks) for _ in range(blocks)]
        for _ in range(40):
            vals = S.draw(rng, blocks)
            want = S.coset_combine(1, blocks, vals, mat)
            got = S.chain_coset_combine(A, blocks, [S.word(v) for v in vals],
                                        [[S.word(x, -1) for x in row] for row in mat])
            assert got == [S.word(x) for x in want]
    for count in (1, 2, 3, 4):
        for _ in range(40):
            l1, v = S.draw(rng, count), S.draw(rng, count)
            want = sum(x * y for x, y in zip(l1, v)) % r
            assert S.chain_pi_sparse(A, count, [S.word(x) for x in l1], [S.word(x) for x in v]) == S.word(want, 1)
    for terms in (1, 2, 24):
        for _ in range(20):
            s, p = S.draw(rng, terms), S.draw(rng, terms)
            present = [None if rng.random() < 0.2 else S.word(x) for x in p]
            want = sum(x * y for x, y, q in zip(s, p, present) if q is not None) % r
            assert S.chain_lincomb(A, terms, [S.word(x, -1) for x in s], present) == S.word(want)


@pytest.mark.parametrize("threads,length,block", [(256, 4096, 0), (256, 300, 1), (8, 128, 5), (8, 77, 2), (8, 1, 0)])
def test_concrete_eval_block_equals_horner(threads, length, block):
    import pyref as P
    rng = random.Random(length)
    size = threads * S.EVAL_PER
    for x in (0, 1, r - 1, 2, rng.randrange(r), pow(P.omega(12), 4096 // size, r)) if threads == 8 else (rng.randrange(r),):
        coef = S.draw(rng, length)
        want = P.poly_eval(coef, x) * pow(x, block * size, r) % r
        got = S.chain_eval_block(S.Concrete(), [S.word(c) for c in coef], S.word(x, -1), block, threads=threads)
        assert got == S.word(want), (x, threads, length, block)


def test_model_rejects_weakened_chains():
    """rx_sub_u<3> modelled as <2> (a limb can go negative), seven carry-free summands where the
    kernel has four (a column can reach 2^64), and the first add3_u factor left unnormalised."""
    S.chain_quotient(S.Bounds(), None, None)
    with pytest.raises(AssertionError, match="negative"):
        S.chain_quotient(S.Bounds(), None, None, cp=2)
    with pytest.raises(AssertionError, match="column"):
        S.chain_quotient(S.Bounds(), None, None, extra_summands=3)
    with pytest.raises(AssertionError, match="column"):
        S.chain_quotient(S.Bounds(), None, None, drop_norm=True)
    # the concrete model at the operand that breaks <2>: 0 + 2r - (2r - 1) borrows in the top limb
    A = S.Concrete()
    assert F.value(A.sub_u(F.limbs(0), F.limbs(2 * r - 1), 3)) == r + 1
    with pytest.raises(AssertionError, match="32 bits"):
        A.sub_u(F.limbs(0), F.limbs(2 * r - 1), 2)
    # a non-canonical word is outside the input contract
    with pytest.raises(AssertionError, match="canonical"):
        A.ld(r)
    # and the product bound: 9r x 9r leaves [0, 2r)
    with pytest.raises(AssertionError, match="product"):
        S.Bounds().mul(S.Bounds.below(9), S.Bounds.below(9))
