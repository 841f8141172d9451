"""pk_scan (csrc/prover_kernels.hip) through plk_debug_prover_stage: all eight (multiply | add,
prefix | suffix, inclusive | exclusive) forms, in place (as the prover scans) and out of place, the
outputs and the grand total the prover reads at tmp[blocks] against plain Python prefix / suffix
products and sums, at the lengths where the code changes path: 1 024 | 1 025 (k_scan_single's
elements per thread 1 -> 2), 32 768 | 32 769 (k_scan_single -> the three-phase form), 34 817 (18
blocks, a ragged last one) and, for the three forms the prover uses, 524 288 | 524 289
(k_scan_tops' blocks per thread 1 -> 2, with a one-element last block)."""
from __future__ import annotations

import functools
import random

import numpy as np
import pytest

import prover_stage_ref as S

pytestmark = pytest.mark.gpu
r = S.r
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 32767, 32768, 32769, 34817)
BIG = (524288, 524289)
# (mul, suffix, exclusive) of the prover: N_i = prod_{j<i}, S_i = prod_{j>=i}, Ruffini's sum_{i>j}
PROVER_FORMS = ((True, False, True), (True, True, False), (False, True, True))
PRODUCT_DATA = ("random", "minus_one", "zero_first", "zero_middle", "zero_last", "ones")
SUM_DATA = ("minus_one", "random")


@functools.lru_cache(maxsize=None)
def data(kind: str, n: int) -> tuple:
    """(plain values, their ABI array); computed once per module and left unchanged."""
    if kind == "random":
        rng = random.Random(n)
        vals = [rng.randrange(1, r) for _ in range(n)]
    elif kind == "minus_one":
        vals = [r - 1] * n
    elif kind == "ones":
        vals = [1] * n
    else:
        rng = random.Random(n + 1)
        vals = [rng.randrange(1, r) for _ in range(n)]
        vals[{"zero_first": 0, "zero_middle": n // 2, "zero_last": n - 1}[kind]] = 0
    arr = S.words_np(vals)
    arr.setflags(write=False)
    return vals, arr


@functools.lru_cache(maxsize=None)
def reference(kind: str, n: int, mul: bool, suffix: bool) -> tuple:
    """(inclusive outputs, exclusive outputs, total word) as ABI arrays, from ONE scan."""
    vals, _ = data(kind, n)
    incl, total = S.scan(vals, mul, suffix, False)
    ident = 1 if mul else 0
    excl = incl[1:] + [ident] if suffix else [ident] + incl[:-1]
    return S.words_np(incl), S.words_np(excl), S.words_np([total])


def check(ctx, kind, n, mul, suffix, exclusive):
    vals, arr = data(kind, n)
    incl, excl, total = reference(kind, n, mul, suffix)
    want = excl if exclusive else incl
    for in_place in (True, False):
        flags = (1 if mul else 0) | (2 if suffix else 0) | (4 if exclusive else 0) | (8 if in_place else 0)
        got = ctx.prover_stage("scan", [arr], params=[flags], out_len=n + 1)
        what = f"n={n} data={kind} mul={mul} suffix={suffix} exclusive={exclusive} in_place={in_place}"
        bad = np.nonzero((got[:n] != want).any(axis=1))[0]
        assert bad.size == 0, f"{what}: outputs differ first at {bad[:4]}"
        assert np.array_equal(got[n:], total), f"{what}: grand total"


@pytest.mark.parametrize("n", SIZES)
def test_all_eight_scan_forms(gpu_ctx, n):
    for mul in (True, False):
        for kind in (PRODUCT_DATA if mul else SUM_DATA):
            for suffix in (False, True):
                for exclusive in (False, True):
                    check(gpu_ctx, kind, n, mul, suffix, exclusive)


@pytest.mark.parametrize("form", PROVER_FORMS, ids=("prefix_excl_product", "suffix_incl_product", "suffix_excl_sum"))
@pytest.mark.parametrize("n", BIG)
def test_prover_scan_forms_where_the_block_totals_take_two_per_thread(gpu_ctx, n, form):
    mul, suffix, exclusive = form
    for kind in (PRODUCT_DATA if mul else SUM_DATA):
        check(gpu_ctx, kind, n, mul, suffix, exclusive)


def test_scan_of_nothing_is_ok(gpu_ctx):
    assert gpu_ctx.prover_stage("scan", [np.zeros((0, 4), np.uint64)], params=[1], out_len=0).shape == (0, 4)
