"""pk_eval, pk_lincomb, pk_ruffini and pk_scale_powers (csrc/prover_kernels.hip) through
plk_debug_prover_stage against Horner evaluation, the plain linear combination and the classical
top-down synthetic division (pyref.ruffini), at the lengths where the code changes path: the 4 096
coefficient blocks of k_eval_partial / k_scale_powers (and whole blocks past a short polynomial's
end inside a mixed batch), k_ruffini_single's elements per thread stepping at multiples of 1 024
up to its limit 16 384, and the five-dispatch form above it."""
from __future__ import annotations

import functools
import random

import numpy as np
import pytest

import prover_stage_ref as S
import pyref as P
from oracle_lib import random_fr

pytestmark = pytest.mark.gpu
r = S.r
EVAL_LENS = (0, 1, 255, 256, 257, 4095, 4096, 4097, 8192, 12293)
RUFFINI_LENS = (2, 3, 1023, 1024, 1025, 2048, 2049, 16383, 16384, 16385, 20479, 20480, 20481, 32769, 32770)


def points(seed: int) -> list:
    """0, 1, r - 1, 2, a random value and roots of unity of order 256 and 4 096 (x^256 = 1 folds
    the in-block Horner steps onto one power, x^4096 = 1 every block-start power)."""
    return [0, 1, r - 1, 2, random.Random(seed).randrange(r), P.omega(8), P.omega(12)]


@functools.lru_cache(maxsize=None)
def poly(length: int, kind: str = "random") -> tuple:
    if kind == "minus_one":
        vals = [r - 1] * length
    else:
        rng = random.Random(1000 + length)
        vals = [rng.randrange(r) for _ in range(length)]
    arr = S.words_np(vals) if length else np.zeros((0, 4), np.uint64)
    arr.setflags(write=False)
    return vals, arr


@pytest.mark.parametrize("length", EVAL_LENS)
def test_eval_single_polynomial(gpu_ctx, length):
    vals, arr = poly(length)
    for x in points(length):
        got = gpu_ctx.prover_stage("eval", [arr], S.words_np([x]), out_len=1)
        assert np.array_equal(got, S.words_np([P.poly_eval(vals, x)])), (length, x)


def test_eval_batch_of_28_mixed_lengths_each_at_its_own_point(gpu_ctx):
    """The longest polynomial sets the grid (4 blocks): the short ones leave 1 to 4 whole blocks
    past their end, which must contribute zero."""
    lens = [12293, 0, 1, 255, 4096, 4097, 8192, 5, 256, 257, 4095, 8193, 12288, 12289, 2, 100,
            4096, 1, 0, 9000, 300, 8191, 12293, 7, 4097, 1024, 16, 12292]
    assert len(lens) == 28
    pts = (points(28) * 4)[:28]
    pts[22] = P.omega(12)  # the longest again, where every block-start power is 1
    polys = [poly(m) for m in lens]
    got = gpu_ctx.prover_stage("eval", [p[1] for p in polys], S.words_np(pts), out_len=28)
    want = [P.poly_eval(p[0], x) for p, x in zip(polys, pts)]
    assert np.array_equal(got, S.words_np(want))
    assert gpu_ctx.prover_stage("eval", [], [], out_len=0).shape == (0, 4)


def test_eval_refuses_more_polynomials_than_a_batch_holds(plk, gpu_ctx):
    with pytest.raises(plk.PlonkError) as e:
        gpu_ctx.prover_stage("eval", [poly(5)[1]] * 29, S.words_np([2] * 29), out_len=29)
    assert e.value.status == plk.PLK_E_ARG


@pytest.mark.parametrize("terms", (1, 2, 24))
def test_lincomb(gpu_ctx, terms):
    rng = random.Random(terms)
    lens = [rng.choice((0, 1, 255, 256, 257, 700)) for _ in range(terms)]
    lens[0] = 700
    if terms > 1:
        lens[1] = 0  # a term of length 0
    polys = [S.draw(rng, m) for m in lens]
    len_out = 777  # longer than every term: the tail is zero
    for scalars in (S.draw(rng, terms), [0] * terms, [r - 1] * terms,
                    [(0, r - 1)[t & 1] for t in range(terms)]):
        arrays = [S.words_np(p) if p else np.zeros((0, 4), np.uint64) for p in polys]
        got = gpu_ctx.prover_stage("lincomb", arrays, S.words_np(scalars), [len_out], len_out)
        assert np.array_equal(got, S.words_np(S.lincomb(polys, scalars, len_out))), terms
    assert gpu_ctx.prover_stage("lincomb", [S.words_np([1])], S.words_np([1]), [0], 0).shape == (0, 4)


def ruffini_points(seed):
    return [1, r - 1, 2, random.Random(seed).randrange(1, r), P.omega(10)]


@pytest.mark.parametrize("length", RUFFINI_LENS)
def test_ruffini_through_the_stage_hook(gpu_ctx, length):
    u = random.Random(length).randrange(r)
    for kind in ("random", "minus_one"):
        vals, arr = poly(length, kind)
        pu = P.poly_eval(vals, u)
        for z in ruffini_points(length):
            got = gpu_ctx.prover_stage("ruffini", [arr], S.words_np([z]), out_len=length - 1)
            q = P.ruffini(vals, z)
            assert np.array_equal(got, S.words_np(q)), (length, kind, z)
            # q(X)(X - z) + p(z) == p(X) at one random point
            qv = [v * P.FR_RINV % r for v in S.from_np(got)]
            assert (P.poly_eval(qv, u) * (u - z) + P.poly_eval(vals, z)) % r == pu


@pytest.mark.parametrize("length", RUFFINI_LENS)
def test_ruffini_through_the_aggregate_witness(plk, gpu_ctx, length):
    pp = plk.PlonkParams.setup(4, random_fr(1, seed=1)[0], gpu_ctx)
    vals, arr = poly(length)
    for z in ruffini_points(length)[2:]:
        got = pp.compute_aggregate_witness([np.array(arr)], S.words_np([z]), S.words_np([1])).values
        assert np.array_equal(got, S.words_np(P.ruffini(vals, z))), (length, z)


@pytest.mark.parametrize("length", RUFFINI_LENS)
def test_scale_powers(gpu_ctx, length):
    vals, arr = poly(length)
    for shift in (0, 1):
        for x in ruffini_points(length):
            got = gpu_ctx.prover_stage("scale_powers", [arr], S.words_np([x]), [shift], length)
            assert np.array_equal(got, S.words_np(S.scale_powers(vals, x, shift))), (length, shift, x)


def test_ruffini_of_a_constant_is_empty_and_zero_point_is_refused(plk, gpu_ctx):
    assert gpu_ctx.prover_stage("ruffini", [S.words_np([5])], S.words_np([2]), out_len=0).shape == (0, 4)
    with pytest.raises(plk.PlonkError) as e:
        gpu_ctx.prover_stage("ruffini", [S.words_np([5, 6, 7])], S.words_np([0]), out_len=2)
    assert e.value.status == plk.PLK_E_ARG
